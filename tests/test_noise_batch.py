"""Host side of the batched device noise path (datasets/pdbbind.py: NoiseTransform.draw, the packing of the ragged batch for
cbd_noise_conformers; finetune_train._Loader's batch_transform).  No GPU: the draws, the generators and the packed arrays are host data."""
import copy
import random
from functools import partial

import numpy as np
import pytest
import torch

from tests.noise_helpers import rot_edges, tree_ligand

SHAPES = [(12, 3), (7, 0), (1, 0), (33, 7), (5, 1), (20, 9)]      # (Nl, R): mixed R, one rigid ligand, one single atom


def _t_to_sigma():
    from confidence_bootstrapping_amd.diffusion_utils import t_to_sigma
    from confidence_bootstrapping_amd.utils import load_model_args
    return partial(t_to_sigma, args=load_model_args())


def _items():
    return [tree_ligand(nl, r, seed=40 + i) for i, (nl, r) in enumerate(SHAPES)]


def _seed(s):
    np.random.seed(s)
    torch.manual_seed(s)
    random.seed(s)


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("kw", [dict(), dict(separate_noise_schedule=True, alpha=2, beta=3, rot_alpha=1, rot_beta=2, tor_alpha=3, tor_beta=1),
                                dict(sampling_mixing_coeff=0.4, minimum_t=0.1), dict(no_torsion=True)],
                         ids=["common_t", "separate_schedule", "mixing", "no_torsion"])
def test_draw_consumes_the_generators_like_sequential_calls(kw, monkeypatch):
    from confidence_bootstrapping_amd.datasets import pdbbind
    kw = dict(kw)
    nt = pdbbind.NoiseTransform(t_to_sigma=_t_to_sigma(), no_torsion=kw.pop("no_torsion", False), all_atom=False, **kw)
    # the old way: __call__ per item on copies; the updates are what it hands to modify_conformer
    seen = []
    real = pdbbind.modify_conformer

    def spy(data, tr_update, rot_update, torsion_updates):
        seen.append((tr_update, rot_update, torsion_updates))
        return real(data, tr_update, rot_update, torsion_updates)
    monkeypatch.setattr(pdbbind, "modify_conformer", spy)
    _seed(7)
    old = [nt(copy.deepcopy(g)) for g in _items()]
    state_old = (np.random.get_state(), torch.get_rng_state(), random.getstate())
    monkeypatch.setattr(pdbbind, "modify_conformer", real)
    # the new way: draw per item, poses untouched
    _seed(7)
    new = _items()
    before = [g["ligand"].pos.clone() for g in new]
    drawn = [nt.draw(g) for g in new]
    state_new = (np.random.get_state(), torch.get_rng_state(), random.getstate())
    assert len(seen) == len(SHAPES)
    for g_old, g_new, (tr_o, rot_o, tor_o), (tr_n, rot_n, tor_n), pos0 in zip(old, new, seen, drawn, before):
        assert torch.equal(g_new["ligand"].pos, pos0)                      # draw does not move the pose
        for k in ("tr", "rot", "tor"):
            assert _same(g_old.complex_t[k], g_new.complex_t[k])
            assert _same(g_old["ligand"].node_t[k], g_new["ligand"].node_t[k])
        for f in ("tr_score", "rot_score", "tor_score", "tor_sigma_edge"):
            assert _same(getattr(g_old, f), getattr(g_new, f)), f
        assert _same(tr_o, tr_n) and _same(rot_o, torch.from_numpy(rot_n).float()) and _same(tor_o, tor_n)
    assert torch.count_nonzero(new[2].rot_score) == 0 and torch.count_nonzero(new[0].rot_score) == 3      # the single-atom rule
    so, sn = state_old[0], state_new[0]
    assert so[0] == sn[0] and np.array_equal(so[1], sn[1]) and so[2:] == sn[2:]
    assert torch.equal(state_old[1], state_new[1]) and state_old[2] == state_new[2]


@pytest.mark.parametrize("nl,r", [(33, 7), (65, 33), (5, 1), (1, 0), (32, 3), (64, 5)])
def test_packed_mask_and_edges_reproduce_mask_rotate(nl, r):
    """Nl = 33 and 65 cross the first and second 32-bit word boundary of a mask row, R = 33 that of the bond count; 32 and 64 end on one."""
    from confidence_bootstrapping_amd.datasets.pdbbind import pack_ligand, pack_mask_rotate, unpack_mask_rotate
    g = tree_ligand(nl, r, seed=3)
    edges, bits = pack_ligand(g)
    words = (nl + 31) // 32
    assert edges.dtype == np.int32 and edges.shape == (r, 2) and bits.dtype == np.uint32 and bits.shape == (r, words)
    assert np.array_equal(edges, rot_edges(g))
    mask = np.asarray(g["ligand"].mask_rotate, dtype=bool).reshape(r, nl)
    assert np.array_equal(unpack_mask_rotate(bits, nl), mask)
    for k in range(r):                      # the layout the kernel reads: atom a = bit a % 32 of word a // 32
        for a in range(nl):
            assert (int(bits[k, a >> 5]) >> (a & 31)) & 1 == int(mask[k, a])
        if nl % 32:
            assert int(bits[k, -1]) >> (nl % 32) == 0                      # padding bits are clear
    if r:
        assert mask.any(axis=1).all() and not mask.all(axis=1).any()
        # a bond's v end turns with its side, its u end does not (the rotation is about pos[u] - pos[v] through pos[v])
        assert all(mask[k, edges[k, 1]] and not mask[k, edges[k, 0]] for k in range(r))
    rnd = np.random.default_rng(0).random((r, nl)) < 0.5
    assert np.array_equal(unpack_mask_rotate(pack_mask_rotate(rnd), nl), rnd)


def test_packed_ligand_is_cached_per_ligand_identity():
    from confidence_bootstrapping_amd.datasets.pdbbind import NoiseTransform
    nt = NoiseTransform(t_to_sigma=_t_to_sigma(), no_torsion=False, all_atom=False)
    g, other = tree_ligand(12, 3, seed=1), tree_ligand(12, 3, seed=2)
    a = nt._packed(g)
    assert nt._packed(g.shallow_copy()) is a                               # the buffer's copies share the ligand's arrays
    b = nt._packed(other)
    assert b is not a and not np.array_equal(a[1], b[1])
    assert nt._packed(copy.deepcopy(g)) is not a                           # another object: packed again, same contents
    assert np.array_equal(nt._packed(copy.deepcopy(g))[1], a[1])


def test_apply_noise_batch_has_no_cpu_path():
    from confidence_bootstrapping_amd.datasets.pdbbind import NoiseTransform
    nt = NoiseTransform(t_to_sigma=_t_to_sigma(), no_torsion=False, all_atom=False)
    with pytest.raises(RuntimeError, match="MI355X"):
        nt.apply_noise_batch([tree_ligand(5, 1, seed=1)], "cpu")
    for bad in (dict(all_atom=True), dict(asyncronous_noise_schedule=True), dict(time_independent=True), dict(crop_beyond_cutoff=5.0)):
        args = dict(t_to_sigma=_t_to_sigma(), no_torsion=False, all_atom=False)
        args.update(bad)
        with pytest.raises(NotImplementedError):
            NoiseTransform(**args)


def test_loader_with_batch_transform_keeps_the_item_order():
    from confidence_bootstrapping_amd.bootstrapping.buffer import CBBuffer
    from confidence_bootstrapping_amd.finetune_train import _Loader
    names = [f"{1000 + i}_A_l{i}" for i in range(7)]
    buf = CBBuffer(cluster_name="c", cluster_to_ligands={"c": names}, transform=lambda g: g)
    buf.add_complexes([(tree_ligand(4 + i, 0, seed=i, name=n), 0.1 * i) for i, n in enumerate(names)])
    calls = []

    def whole_batch(items):
        calls.append(len(items))
        return items
    np.random.seed(5)
    plain = [[g.name for g in batch] for batch in _Loader(buf, 3)]
    np.random.seed(5)
    batched = [[g.name for g in batch] for batch in _Loader(buf, 3, batch_transform=whole_batch)]
    assert plain == batched and calls == [3, 3, 1] and sorted(sum(plain, [])) == sorted(names)
    np.random.seed(5)
    assert [[g.name for g in b] for b in _Loader(buf, 3, drop_last=True, batch_transform=whole_batch)] == plain[:2]
    assert len(_Loader(buf, 3, batch_transform=whole_batch)) == 3
