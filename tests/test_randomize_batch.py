"""Host side of the batched device randomisation of starting poses (sampling.py: draw_randomization, the packing of the ragged batch
for cbd_randomize_poses, randomize_position_batch's failure modes).  No GPU: the draws, the generators and the packed arrays are host
data."""
import copy

import numpy as np
import pytest
import torch

from tests.randomize_helpers import graph_arrays, randomize64_list, rot_edges, tree_ligand


def _seed(s):
    np.random.seed(s)
    torch.manual_seed(s)


def _states():
    return np.random.get_state(), torch.get_rng_state()


def _same_states(a, b):
    return a[0][0] == b[0][0] and np.array_equal(a[0][1], b[0][1]) and a[0][2:] == b[0][2:] and torch.equal(a[1], b[1])


def test_draws_fed_to_the_fp64_restatement_reproduce_the_reference_golden(golden):
    """the workloads, seeds and tolerance of tests/test_host_api.py::test_randomize_position_matches_reference: pins the draw order and
    the restatement to poses the reference produced"""
    from confidence_bootstrapping_amd import Batch
    from confidence_bootstrapping_amd.sampling import draw_randomization
    from confidence_bootstrapping_amd.synthetic import make_workload
    g = golden("g7_randomize.npz")
    for wl in ("tiny", "c2_dockgen_median"):
        cplx = make_workload(wl)
        dl = [Batch.from_data_list([copy.deepcopy(cplx)]) for _ in range(4)]
        before = [d["ligand"].pos.clone() for d in dl]
        _seed(7)
        draws = draw_randomization(dl, False, False, 19.0)
        assert all(torch.equal(d["ligand"].pos, b) for d, b in zip(dl, before))          # drawing moves nothing
        tor, rot_mat, tr = draws
        n_tor = int(cplx["ligand"].edge_mask.sum())
        assert len(tor) == 4 and all(t.dtype == np.float64 and t.shape == (n_tor,) for t in tor)
        assert rot_mat.dtype == torch.float32 and rot_mat.shape == (4, 3, 3) and tr.dtype == torch.float32 and tr.shape == (4, 1, 3)
        center = dl[0]["receptor"].pos.numpy().astype(np.float64).mean(0)
        got = np.stack(randomize64_list(dl, center, draws))
        want = g[f"{wl}_pos"].astype(np.float64)
        err = float(np.abs(got - want).max())
        print(f"\n{wl}: fp64 restatement on draw_randomization's draws vs the reference's golden: max |err| {err:.2e} A")
        assert got.shape == want.shape and err <= 2e-5


@pytest.mark.parametrize("no_torsion", [False, True])
@pytest.mark.parametrize("no_random", [False, True])
def test_generator_states_after_drawing_equal_those_after_randomize_position(no_torsion, no_random):
    from confidence_bootstrapping_amd.sampling import _pocket_center, _randomize_with_draws, draw_randomization, randomize_position
    ligs = [tree_ligand(12, 3, seed=1), tree_ligand(7, 0, seed=2), tree_ligand(1, 0, seed=3), tree_ligand(20, 9, seed=4)]
    old = [g.shallow_copy() for g in ligs]
    _seed(11)
    randomize_position(old, no_torsion, no_random, 19.0)
    after_old = _states()
    new = [g.shallow_copy() for g in ligs]
    _seed(11)
    draws = draw_randomization(new, no_torsion, no_random, 19.0)
    after_new = _states()
    assert _same_states(after_old, after_new)
    assert (draws[0] is None) == no_torsion and (draws[2] is None) == no_random
    # the private host route with these draws IS randomize_position: bitwise the same poses
    _randomize_with_draws(new, _pocket_center(new), *draws)
    assert _same_states(after_new, _states())                                          # it draws nothing itself
    for a, b in zip(old, new):
        assert b["ligand"].pos.dtype == torch.float32 and torch.equal(a["ligand"].pos, b["ligand"].pos)


def _bits_by_hand(mask):
    r, nl = mask.shape
    words = np.zeros((r, (nl + 31) // 32), dtype=np.uint32)
    for k in range(r):
        for a in range(nl):
            if mask[k, a]:
                words[k, a // 32] |= np.uint32(1 << (a % 32))
    return words.reshape(-1)


def test_packing_of_two_groups_with_and_without_shared_start_coordinates():
    from confidence_bootstrapping_amd.sampling import _pack_randomization, draw_randomization
    small, big = tree_ligand(5, 1, seed=21), tree_ligand(33, 7, seed=22)
    group_a = [small.shallow_copy() for _ in range(3)]                 # copies of one complex: one description
    group_b = [big.shallow_copy() for _ in range(2)]                   # distinct start coordinates: one description per pose
    group_b[1]["ligand"].pos = big["ligand"].pos + 0.25
    groups = [group_a, group_b]
    centers = [torch.tensor([1.0, 2.0, 3.0]), torch.tensor([-4.0, 5.0, -6.0])]
    _seed(3)
    draws = [draw_randomization(g, False, False, 5.0) for g in groups]
    pk = _pack_randomization(groups, centers, draws)
    i32 = lambda *v: np.asarray(v, dtype=np.int32)
    for name, want in (("pose_lig", i32(0, 0, 0, 1, 2)), ("pose_cplx", i32(0, 0, 0, 1, 1)), ("out_ptr", i32(0, 5, 10, 15, 48, 81)),
                       ("tor_ptr", i32(0, 1, 2, 3, 10, 17)), ("lig_ptr", i32(0, 5, 38, 71)), ("rot_ptr", i32(0, 1, 8, 15)),
                       ("mask_ptr", i32(0, 1, 15, 29))):
        assert pk[name].dtype == np.int32 and np.array_equal(pk[name], want), (name, pk[name])
    assert pk["max_nl"] == 33 and pk["max_r"] == 7
    descs = [small, group_b[0], group_b[1]]
    assert pk["pos_in"].dtype == np.float32 and np.array_equal(pk["pos_in"], np.concatenate([d["ligand"].pos.numpy() for d in descs]))
    assert pk["rot_edge"].dtype == np.int32 and np.array_equal(pk["rot_edge"], np.concatenate([rot_edges(d) for d in descs]))
    assert pk["mask_bits"].dtype == np.uint32
    assert np.array_equal(pk["mask_bits"], np.concatenate([_bits_by_hand(graph_arrays(d)[2]) for d in descs]))
    assert pk["tor"].dtype == np.float64 and np.array_equal(pk["tor"], np.concatenate([t for d in draws for t in d[0]]))
    assert pk["rot_mat"].dtype == np.float32 and np.array_equal(pk["rot_mat"], torch.cat([d[1] for d in draws]).numpy().reshape(5, 9))
    assert pk["tr"].dtype == np.float32 and np.array_equal(pk["tr"], torch.cat([d[2] for d in draws]).numpy().reshape(5, 3))
    assert np.array_equal(pk["center"], np.asarray([[1, 2, 3], [-4, 5, -6]], dtype=np.float32))
    # deep copies of one complex are equal, not identical: still one description; no_torsion / no_random leave their parts out
    group_c = [copy.deepcopy(small) for _ in range(2)]
    pk = _pack_randomization([group_c], centers[:1], [draw_randomization(group_c, True, True, 5.0)])
    assert np.array_equal(pk["pose_lig"], i32(0, 0)) and np.array_equal(pk["lig_ptr"], i32(0, 5)) and pk["tor"] is None and pk["tr"] is None


def test_randomize_position_batch_has_no_cpu_path():
    from confidence_bootstrapping_amd.sampling import randomize_position_batch
    with pytest.raises(RuntimeError, match="MI355X"):
        randomize_position_batch([[tree_ligand(5, 1, seed=1)]], False, False, 5.0, device="cpu")


def test_a_group_over_the_capacity_takes_the_host_route_with_its_draws_in_order():
    """both groups are over the capacity (R = 129 > 128, Nl = 513 > 512), so nothing reaches the GPU and the call runs without one; the
    poses and the generators must be what randomize_position leaves group after group"""
    from confidence_bootstrapping_amd.sampling import RANDOMIZE_MAX_ATOMS, RANDOMIZE_MAX_TORSIONS, randomize_position, randomize_position_batch
    many_bonds, many_atoms = tree_ligand(230, RANDOMIZE_MAX_TORSIONS + 1, seed=9), tree_ligand(RANDOMIZE_MAX_ATOMS + 1, 2, seed=10)
    old = [[g.shallow_copy() for _ in range(2)] for g in (many_bonds, many_atoms)]
    _seed(5)
    for dl in old:
        randomize_position(dl, False, False, 7.0)
    after_old = _states()
    new = [[g.shallow_copy() for _ in range(2)] for g in (many_bonds, many_atoms)]
    _seed(5)
    assert randomize_position_batch(new, False, False, 7.0, device="cuda:0") is new
    assert _same_states(after_old, _states())
    for dl_old, dl_new in zip(old, new):
        for a, b in zip(dl_old, dl_new):
            assert not b["ligand"].pos.is_cuda and torch.equal(a["ligand"].pos, b["ligand"].pos)
    assert not torch.equal(new[0][0]["ligand"].pos, many_bonds["ligand"].pos)
