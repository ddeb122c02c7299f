"""cbd_randomize_poses (csrc/randomize_poses.hip) through sampling.randomize_position_batch: one launch over the poses of ligands of
different Nl, R and mask_rotate against an fp64 numpy restatement of randomize_position (tests/randomize_helpers.py).

The bound is not a chosen number: it is 4 x the largest deviation of the existing host `randomize_position` arithmetic
(sampling._randomize_with_draws, fed the same prescribed draws) from that same fp64 restatement on these same inputs -- both paths work
on fp32 coordinates with their own summation order -- and each invariant gets 4 x the host path's own deviation from it.
The host path's figures on these inputs (host code only): 4.0e-6 A against fp64, bond lengths 1.8e-6 A, centroid vs center + tr
1.2e-6 A, tor null vs the rigid image 1.5e-6 A, tr null centroid 1.0e-6 A; the tests print both sides' figures before they assert
(DESIGN.md section 8)."""
import copy
import ctypes as C
import os
from argparse import Namespace
from functools import partial

import numpy as np
import pytest
import torch

from tests.randomize_helpers import bonds_of, randomize64_list, tree_ligand

pytestmark = pytest.mark.gpu
SDF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "1a0q", "1a0q_ligand.sdf")
SHAPES = [(1, 0), (2, 0), (5, 1), (33, 7), (65, 33)]          # + the 1a0q ligand (23 atoms, 11 rotatable bonds)
POSES = 3
DISTINCT = 3                                                  # the group whose poses have distinct start coordinates


def _ligands():
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    ligs = [tree_ligand(nl, r, seed=200 + i) for i, (nl, r) in enumerate(SHAPES)]
    g = pm.get_ligand(SDF, "1a0q")
    g["ligand"].pos = g["ligand"].pos.float() - g["ligand"].pos.float().mean(0) + torch.tensor([3.0, -8.0, 11.0])
    g["receptor"].pos = torch.tensor([[14.0, -2.5, 7.25], [10.0, 1.5, 3.75]])
    return ligs + [g]


def _groups(ligs):
    """POSES shallow copies per ligand; the poses of group DISTINCT start from different coordinates"""
    rng = np.random.default_rng(5)
    groups = [[g.shallow_copy() for _ in range(POSES)] for g in ligs]
    for d in groups[DISTINCT][1:]:
        d["ligand"].pos = d["ligand"].pos + torch.from_numpy(rng.normal(0, 0.1, size=tuple(d["ligand"].pos.shape)).astype(np.float32))
    return groups


def _draws(ligs):
    """draw_randomization's triple per group; every value is exactly representable in fp32, so that every path is given the same numbers.
    Special values: a torsion update of exactly 0 (groups 3 and 5), one equal to (fp32) pi (group 4), tr = 0 (pose 1 of group 4), the
    identity rotation (pose 0 of group 2) and a 180 degree rotation (pose 2 of group 3)."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(23)
    out = []
    for i, g in enumerate(ligs):
        r = int(g["ligand"].edge_mask.sum())
        tor = [rng.uniform(-np.pi, np.pi, size=r).astype(np.float32).astype(np.float64) for _ in range(POSES)]
        rot = torch.from_numpy(Rotation.random(POSES, random_state=100 + i).as_matrix()).float()
        tr = torch.from_numpy(rng.normal(0, 5, size=(POSES, 1, 3)).astype(np.float32))
        if i == 2:
            rot[0] = torch.eye(3)
        if i == 3:
            tor[0][3] = 0.0
            rot[2] = torch.diag(torch.tensor([-1.0, -1.0, 1.0]))
        if i == 4:
            tor[1][5] = float(np.float32(np.pi))
            tr[1] = 0.0
        if i == 5:
            tor[2][0] = 0.0
        out.append((tor, rot, tr))
    return out


def _launch(groups, draws, dev, monkeypatch_ctx, no_torsion=False, no_random=False):
    """randomize_position_batch on fresh copies of `groups` with the draws prescribed -> list of lists of CPU fp32 positions"""
    import confidence_bootstrapping_amd.sampling as smp
    items = [[g.shallow_copy() for g in group] for group in groups]
    table = {id(group): (None if no_torsion else d[0], d[1], None if no_random else d[2]) for group, d in zip(items, draws)}
    with monkeypatch_ctx() as mp:
        mp.setattr(smp, "draw_randomization", lambda data_list, *a, **k: table[id(data_list)])
        smp.randomize_position_batch(items, no_torsion, no_random, 5.0, dev)
    return [[g["ligand"].pos for g in group] for group in items]


def _host(groups, draws, no_torsion=False, no_random=False):
    """the existing host arithmetic with the same draws -> float64 arrays"""
    from confidence_bootstrapping_amd.sampling import _pocket_center, _randomize_with_draws
    out = []
    for group, (tor, rot, tr) in zip(groups, draws):
        items = [g.shallow_copy() for g in group]
        _randomize_with_draws(items, _pocket_center(items), None if no_torsion else tor, rot, None if no_random else tr)
        assert all(g["ligand"].pos.dtype == torch.float32 for g in items)
        out.append([g["ligand"].pos.numpy().astype(np.float64) for g in items])
    return out


def _ref(groups, draws, centers, no_torsion=False, no_random=False):
    return [randomize64_list(group, c, (None if no_torsion else d[0], d[1], None if no_random else d[2]))
            for group, d, c in zip(groups, draws, centers)]


@pytest.fixture(scope="module")
def case():
    """inputs, the fp64 restatement, the host fp32 path, one device launch of everything (and one each with tor / tr null) -- computed once"""
    from confidence_bootstrapping_amd.sampling import _pocket_center
    dev = torch.device("cuda:0")
    ligs = _ligands()
    groups, draws = _groups(ligs), _draws(ligs)
    centers = [_pocket_center(group).numpy() for group in groups]
    ctx = pytest.MonkeyPatch.context
    c = dict(dev=dev, ligs=ligs, groups=groups, draws=draws, centers=centers, ctx=ctx)
    for tag, kw in (("", {}), ("_notor", dict(no_torsion=True)), ("_notr", dict(no_random=True))):
        c["ref" + tag] = _ref(groups, draws, centers, **kw)
        c["host" + tag] = _host(groups, draws, **kw)
        got = _launch(groups, draws, dev, ctx, **kw)
        assert all(not p.is_cuda and p.dtype == torch.float32 and p.shape == g["ligand"].pos.shape
                   for ps, group in zip(got, groups) for p, g in zip(ps, group))
        c["got_t" + tag] = got
        c["got" + tag] = [[p.numpy().astype(np.float64) for p in ps] for ps in got]
    return c


def _worst(outs, refs):
    return [max(float(np.abs(o - r).max()) for o, r in zip(og, rg)) for og, rg in zip(outs, refs)]


def test_every_pose_matches_the_fp64_restatement(case):
    host_err, kern_err = _worst(case["host"], case["ref"]), _worst(case["got"], case["ref"])
    bound = 4 * max(host_err)
    print(f"\nmax |err| vs fp64 per group: host fp32 {['%.2e' % e for e in host_err]} kernel {['%.2e' % e for e in kern_err]} "
          f"bound 4 x {max(host_err):.3e} = {bound:.3e}")
    assert all(np.isfinite(k).all() for ks in case["got"] for k in ks)
    assert max(host_err) < 1e-4            # the yardstick itself is sane (coordinates of tens of A in fp32)
    for i, e in enumerate(kern_err):
        assert e <= bound, (i, e, bound)


def _bond_dev(group, outs):
    worst = 0.0
    for g, out in zip(group, outs):
        b = bonds_of(g)
        if len(b):
            p0 = g["ligand"].pos.numpy().astype(np.float64)
            length = lambda p: np.linalg.norm(p[b[:, 0]] - p[b[:, 1]], axis=1)
            worst = max(worst, float(np.abs(length(out) - length(p0)).max()))
    return worst


def test_invariants_hold_as_well_as_on_the_host_path(case):
    groups, draws, centers = case["groups"], case["draws"], case["centers"]

    def figures(tag):
        outs, notor, notr = case[tag], case[tag + "_notor"], case[tag + "_notr"]
        bond = max(_bond_dev(group, og) for group, og in zip(groups, outs))
        cen = max(float(np.abs(o.mean(0) - (c.astype(np.float64) + d[2][k].numpy().astype(np.float64).reshape(3))).max())
                  for og, d, c in zip(outs, draws, centers) for k, o in enumerate(og))
        rigid = max(_worst(notor, case["ref_notor"]))              # tor null: the rigid image of the input
        cen0 = max(float(np.abs(o.mean(0) - c.astype(np.float64)).max()) for og, c in zip(notr, centers) for o in og)
        return bond, cen, rigid, cen0
    host, kern = figures("host"), figures("got")
    names = ("bond length", "centroid vs center + tr", "tor null: out vs rigid image", "tr null: centroid vs center")
    print(f"\n{names}: host {['%.2e' % e for e in host]} kernel {['%.2e' % e for e in kern]} bounds 4 x host")
    for name, h, k in zip(names, host, kern):
        assert k <= 4 * h, (name, k, 4 * h)


def test_two_launches_are_bitwise_identical(case):
    again = _launch(case["groups"], case["draws"], case["dev"], case["ctx"])
    for ps, qs in zip(case["got_t"], again):
        assert all(torch.equal(p, q) for p, q in zip(ps, qs))


def test_a_group_launched_alone_equals_the_group_among_the_others(case):
    for k in (DISTINCT, 4, 0):
        alone = _launch([case["groups"][k]], [case["draws"][k]], case["dev"], case["ctx"])[0]
        assert all(torch.equal(p, q) for p, q in zip(alone, case["got_t"][k])), k


def test_through_the_api_with_the_seeds_of_the_golden_test(case):
    from confidence_bootstrapping_amd import Batch
    from confidence_bootstrapping_amd.sampling import _pocket_center, draw_randomization, randomize_position, randomize_position_batch
    from confidence_bootstrapping_amd.synthetic import make_workload
    dev = case["dev"]
    make = lambda: [[Batch.from_data_list([copy.deepcopy(make_workload(wl))]) for _ in range(4)] for wl in ("tiny", "c2_dockgen_median")]
    seed = lambda: (np.random.seed(7), torch.manual_seed(7))
    old, new, plain = make(), make(), make()
    seed()
    for dl in old:
        randomize_position(dl, False, False, 19.0)
    state_old = (np.random.get_state(), torch.get_rng_state())
    seed()
    assert randomize_position_batch(new, False, False, 19.0, dev) is new
    state_new = (np.random.get_state(), torch.get_rng_state())
    assert np.array_equal(state_old[0][1], state_new[0][1]) and state_old[0][2:] == state_new[0][2:] and torch.equal(state_old[1], state_new[1])
    seed()
    ref = [randomize64_list(dl, _pocket_center(dl).numpy(), draw_randomization(dl, False, False, 19.0)) for dl in plain]
    for dl, dl_plain in zip(new, plain):
        for g, g0 in zip(dl, dl_plain):
            p = g["ligand"].pos
            assert not p.is_cuda and p.dtype == torch.float32 and p.shape == g0["ligand"].pos.shape
    f64 = lambda groups: [[g["ligand"].pos.numpy().astype(np.float64) for g in dl] for dl in groups]
    host_dev, kern_dev = max(_worst(f64(old), ref)), max(_worst(f64(new), ref))
    apart = max(_worst(f64(new), f64(old)))
    print(f"\nAPI, seeds 7, tr_sigma_max 19: vs fp64 host {host_dev:.2e} device {kern_dev:.2e}; device vs host {apart:.2e}")
    # (device vs host <= the sum of the two deviations is the triangle inequality and cannot fail: printed, not asserted)
    assert kern_dev <= 4 * host_dev


def test_the_launcher_refuses_before_any_launch(case):
    from confidence_bootstrapping_amd import engine
    lib, dev = engine.load_library(), case["dev"]
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)
    zero, ptr = i32(0), i32(0, 1)
    pos, rot, center = torch.zeros(1, 3, device=dev), torch.eye(3, device=dev).reshape(1, 9), torch.zeros(1, 3, device=dev)
    out = torch.full((1, 3), -77.0, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda max_nl, rot_mat: lib.cbd_randomize_poses(1, 1, 1, max_nl, 0, p(zero), p(zero), p(ptr), None, p(ptr), p(pos), None, None, None,
                                                           None, None, rot_mat, None, p(center), p(out), None)
    assert call(513, p(rot)) == -4 and b"512" in lib.cbd_last_error()          # CBD_ERR_CAPACITY
    assert call(1, None) == -1                                                  # CBD_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == -77.0).all())
    assert lib.cbd_randomize_poses(0, 0, 0, 0, 0, *([None] * 16)) == 0          # nothing to do, nothing launched


def test_inference_epoch_fix_with_device_randomize(monkeypatch):
    """tiny workload, 2 complexes x 4 samples x 2 steps, flag off and on under the same seeds: same metric keys, finite values, and the
    starting poses that entered sampling() agree within the API test's bound (each side's deviation from fp64 on these draws)"""
    import confidence_bootstrapping_amd.sampling as smp
    from confidence_bootstrapping_amd.diffusion_utils import t_to_sigma
    from confidence_bootstrapping_amd.synthetic import WORKLOADS, make_complex
    from confidence_bootstrapping_amd.training import inference_epoch_fix
    from confidence_bootstrapping_amd.utils import load_model_args, make_score_model
    dev = torch.device("cuda:0")
    margs = load_model_args()
    model, _ = make_score_model(device=dev, seed=0, args=margs)
    targets = []
    for i in range(2):
        g = make_complex(seed=70 + i, name=f"t{i}", **WORKLOADS["tiny"])
        g["ligand"].orig_pos = g["ligand"].pos.numpy() + g.original_center.numpy()
        nums = np.minimum(g["ligand"].x[:, 0].numpy() + 1, 118)
        g["ligand"].x[:, 0] = torch.from_numpy(nums)
        ei = g["ligand", "ligand"].edge_index.numpy()
        am = np.zeros((len(nums), len(nums)), dtype=int)
        am[ei[0], ei[1]] = 1
        g.mol = Namespace(atomicnums=nums, adjacency_matrix=am)
        targets.append(g)
    t2s = partial(t_to_sigma, args=margs)
    entered, refs = [], []
    real = smp.sampling

    def spy(**kw):
        entered.append([g["ligand"].pos.detach().cpu().clone() for g in kw["data_list"]])
        return real(**kw)
    monkeypatch.setattr(smp, "sampling", spy)

    def with_reference(fn, lists_of):
        """before the real call: the fp64 restatement of every data_list from the generator states of THIS call (sampling() draws its
        step noise from torch's generator between two complexes), then the states are put back"""
        def wrapped(first, no_torsion, no_random, tr_sigma_max, *a, **k):
            states = (np.random.get_state(), torch.get_rng_state())
            for dl in lists_of(first):
                refs.append(randomize64_list(dl, smp._pocket_center(dl).numpy(), smp.draw_randomization(dl, no_torsion, no_random, tr_sigma_max)))
            np.random.set_state(states[0])
            torch.set_rng_state(states[1])
            return fn(first, no_torsion, no_random, tr_sigma_max, *a, **k)
        return wrapped
    monkeypatch.setattr(smp, "randomize_position", with_reference(smp.randomize_position, lambda dl: [dl]))
    monkeypatch.setattr(smp, "randomize_position_batch", with_reference(smp.randomize_position_batch, lambda groups: groups))
    runs = []
    for flag in (False, True):
        args = copy.copy(margs)
        args.__dict__.update(inference_steps=2, inference_samples=4, inference_batch_size=4, inf_pocket_knowledge=False, inf_pocket_cutoff=7,
                             device_randomize=flag)
        torch.manual_seed(7); np.random.seed(7)
        entered.clear()
        refs.clear()
        metrics = inference_epoch_fix(model, targets, dev, t2s, args)
        runs.append((metrics, [list(e) for e in entered], [list(r) for r in refs]))
    (m_off, pos_off, ref_off), (m_on, pos_on, ref_on) = runs
    assert set(m_off) == set(m_on) == {"rmsds_lt2", "rmsds_lt5", "min_rmsds_lt2", "min_rmsds_lt5"}
    assert all(np.isfinite(v) for v in list(m_off.values()) + list(m_on.values()))
    assert len(pos_off) == len(pos_on) == 2 and all(len(e) == 4 for e in pos_off + pos_on)
    assert len(ref_off) == len(ref_on) == 2
    f64 = lambda runs_: [[p.numpy().astype(np.float64) for p in e] for e in runs_]
    host_dev, kern_dev = max(_worst(f64(pos_off), ref_off)), max(_worst(f64(pos_on), ref_on))
    apart = max(_worst(f64(pos_on), f64(pos_off)))
    drift = max(_worst(ref_on, ref_off))
    print(f"\ninference_epoch_fix starting poses: vs fp64 host {host_dev:.2e} device {kern_dev:.2e}; device vs host {apart:.2e}; "
          f"fp64 restatement flag on vs off {drift:.2e}")
    assert all(p.dtype == torch.float32 for e in pos_on for p in e)
    assert host_dev < 1e-4                  # the references are built from the right generator states: the host path matches its own
    # the kernel test's bound, for the flag-on run against the restatement of that run's own draws; and both runs were given the same
    # draws at every call (sampling() of the first complex advances torch's generator alike in both), so the restatements are bitwise
    # equal and the two runs' poses are apart by at most the sum of their deviations (printed above)
    assert kern_dev <= 4 * host_dev
    assert drift == 0.0
