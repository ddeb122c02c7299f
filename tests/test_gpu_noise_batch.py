"""cbd_noise_conformers (csrc/noise_transform.hip) through NoiseTransform.apply_noise_batch: one launch over ligands of different Nl, R
and mask_rotate against an fp64 numpy restatement of modify_conformer (tests/noise_helpers.py).

The bound is not a chosen number: it is 4 x the largest deviation of the existing host fp32 `modify_conformer` from that same fp64
restatement on these same inputs (both paths work on fp32 coordinates with their own summation order; the host runs its torsion
rotations and its Kabsch SVD in fp64, the kernel does not), and each invariant gets 4 x the host path's own deviation from it.
The host path's figures on these inputs (host code only): 2.7e-6 A against fp64, bond lengths 1.7e-6 A, centroid 9.8e-7 A, rigid pose
9.3e-7 A; the tests print both sides' figures before they assert."""
import ctypes as C
import os
from functools import partial

import numpy as np
import pytest
import torch

from tests.noise_helpers import bonds_of, modify_conformer64, rot_edges, tree_ligand

pytestmark = pytest.mark.gpu
SDF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "1a0q", "1a0q_ligand.sdf")
SHAPES = [(1, 0), (2, 0), (5, 1), (33, 7), (65, 33)]          # + the 1a0q ligand (23 atoms, 11 rotatable bonds)


def _t_to_sigma():
    from confidence_bootstrapping_amd.diffusion_utils import t_to_sigma
    from confidence_bootstrapping_amd.utils import load_model_args
    return partial(t_to_sigma, args=load_model_args())


def _transform(updates=None):
    """NoiseTransform whose draws are prescribed (`updates`: id(item) -> (tr, rot, tor)) -- the pose arithmetic is what is under test"""
    from confidence_bootstrapping_amd.datasets.pdbbind import NoiseTransform
    nt = NoiseTransform(t_to_sigma=_t_to_sigma(), no_torsion=False, all_atom=False)
    if updates is not None:
        nt.draw = lambda d: updates[id(d)]
    return nt


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _ligands():
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    ligs = [tree_ligand(nl, r, seed=100 + i) for i, (nl, r) in enumerate(SHAPES)]
    g = pm.get_ligand(SDF, "1a0q")
    g["ligand"].pos = g["ligand"].pos.float() - g["ligand"].pos.float().mean(0) + torch.tensor([3.0, -8.0, 11.0])
    return ligs + [g]


def _updates(ligs):
    """(tr float32 [1, 3], rot float64 [3], tor float64 [R]) per ligand; every value is exactly representable in fp32, so that the host
    path (fp64 torsion updates) and the kernel (fp32) are given the same numbers.  Special values: a torsion update that is exactly 0
    (ligands 3 and 5), |rot| < 1e-6 (ligand 2), |rot| within 1e-3 of pi (ligand 3), tr = 0 (ligand 4)."""
    rng = np.random.default_rng(17)
    ups = []
    for i, g in enumerate(ligs):
        r = int(g["ligand"].edge_mask.sum())
        tr = rng.normal(0, 5, size=(1, 3)).astype(np.float32)
        rot = (_unit(rng) * rng.uniform(0.2, 2.5)).astype(np.float32)
        tor = rng.normal(0, 1.5, size=r).astype(np.float32)
        if i == 2:
            rot = (_unit(rng) * 3e-7).astype(np.float32)
        if i == 3:
            rot = (_unit(rng) * (np.pi - 5e-4)).astype(np.float32)
            tor[3] = 0.0
        if i == 4:
            tr[:] = 0.0
        if i == 5:
            tor[0] = 0.0
        ups.append((torch.from_numpy(tr), rot.astype(np.float64), tor.astype(np.float64)))
    assert np.linalg.norm(ups[2][1]) < 1e-6 and abs(np.linalg.norm(ups[3][1]) - np.pi) < 1e-3
    return ups


def _launch(ligs, ups, dev):
    items = [g.shallow_copy() for g in ligs]
    nt = _transform({id(d): u for d, u in zip(items, ups)})
    nt.apply_noise_batch(items, dev)
    return items


@pytest.fixture(scope="module")
def case():
    """inputs, the fp64 restatement, the host fp32 path and its deviations, one device launch -- computed once"""
    from confidence_bootstrapping_amd.datasets.pdbbind import modify_conformer
    dev = torch.device("cuda:0")
    ligs = _ligands()
    ups = _updates(ligs)
    ref, rigid, host = [], [], []
    for g, (tr, rot, tor) in zip(ligs, ups):
        o, rg = modify_conformer64(g["ligand"].pos.numpy(), rot_edges(g), np.asarray(g["ligand"].mask_rotate).reshape(len(tor), g["ligand"].pos.shape[0]),
                                   tr.numpy(), rot.astype(np.float32), tor)
        ref.append(o)
        rigid.append(rg)
        h = modify_conformer(g.shallow_copy(), tr, torch.from_numpy(rot).float(), tor)["ligand"].pos
        assert h.dtype == torch.float32
        host.append(h.numpy().astype(np.float64))
    items = _launch(ligs, ups, dev)
    torch.cuda.synchronize()
    got = [d["ligand"].pos for d in items]
    assert all(p.is_cuda and p.dtype == torch.float32 and p.shape == g["ligand"].pos.shape for p, g in zip(got, ligs))
    return dict(dev=dev, ligs=ligs, ups=ups, ref=ref, rigid=rigid, host=host, got=[p.cpu().numpy().astype(np.float64) for p in got],
                got_dev=got)


def _bond_dev(g, out):
    b = bonds_of(g)
    if len(b) == 0:
        return 0.0
    p0 = g["ligand"].pos.numpy().astype(np.float64)
    length = lambda p: np.linalg.norm(p[b[:, 0]] - p[b[:, 1]], axis=1)
    return float(np.abs(length(out) - length(p0)).max())


def test_every_ligand_matches_the_fp64_restatement(case):
    host_err = [float(np.abs(h - r).max()) for h, r in zip(case["host"], case["ref"])]
    kern_err = [float(np.abs(k - r).max()) for k, r in zip(case["got"], case["ref"])]
    bound = 4 * max(host_err)
    print(f"\nmax |err| vs fp64 per ligand: host fp32 {['%.2e' % e for e in host_err]} kernel {['%.2e' % e for e in kern_err]} "
          f"bound 4 x {max(host_err):.3e} = {bound:.3e}")
    assert all(np.isfinite(k).all() for k in case["got"])
    assert max(host_err) < 1e-4            # the yardstick itself is sane (coordinates of tens of A in fp32)
    for i, e in enumerate(kern_err):
        assert e <= bound, (i, e, bound)


def test_invariants_hold_as_well_as_on_the_host_path(case):
    ligs = case["ligs"]
    flexible = [i for i, g in enumerate(ligs) if int(g["ligand"].edge_mask.sum()) > 0]
    rigid_only = [i for i in range(len(ligs)) if i not in flexible]
    assert len(flexible) == 4 and len(rigid_only) == 2
    cen = lambda outs, i: float(np.abs(outs[i].mean(0) - case["rigid"][i].mean(0)).max())
    dev_of = lambda outs: (max(_bond_dev(g, o) for g, o in zip(ligs, outs)), max(cen(outs, i) for i in flexible),
                           max(float(np.abs(outs[i] - case["rigid"][i]).max()) for i in rigid_only))
    host, kern = dev_of(case["host"]), dev_of(case["got"])
    print(f"\n(bond length, centroid vs rigid for R > 0, out vs rigid for R = 0): host {['%.2e' % e for e in host]} "
          f"kernel {['%.2e' % e for e in kern]} bounds 4 x host")
    for name, h, k in zip(("bond length", "centroid", "rigid"), host, kern):
        assert k <= 4 * h, (name, k, 4 * h)


def test_two_launches_are_bitwise_identical(case):
    again = _launch(case["ligs"], case["ups"], case["dev"])
    for a, b in zip(case["got_dev"], again):
        assert torch.equal(a, b["ligand"].pos)


def test_permuting_the_ligands_permutes_the_output_bitwise(case):
    perm = [3, 5, 0, 4, 2, 1]
    out = _launch([case["ligs"][k] for k in perm], [case["ups"][k] for k in perm], case["dev"])
    for slot, k in enumerate(perm):
        assert torch.equal(out[slot]["ligand"].pos, case["got_dev"][k]), (slot, k)


def test_an_item_over_the_capacity_is_noised_on_the_host(case):
    from confidence_bootstrapping_amd import engine
    from confidence_bootstrapping_amd.datasets.pdbbind import MAX_TORSIONS, modify_conformer, pack_ligand
    dev = case["dev"]
    big, small = tree_ligand(230, MAX_TORSIONS + 1, seed=9), case["ligs"][2]
    rng = np.random.default_rng(4)
    up_big = (torch.from_numpy(rng.normal(0, 3, size=(1, 3)).astype(np.float32)), rng.normal(0, 1, size=3),
              rng.normal(0, 1, size=MAX_TORSIONS + 1))
    items = _launch([big, small], [up_big, case["ups"][2]], dev)
    want = modify_conformer(big.shallow_copy(), up_big[0], torch.from_numpy(up_big[1]).float(), up_big[2])["ligand"].pos
    assert not items[0]["ligand"].pos.is_cuda and torch.equal(items[0]["ligand"].pos, want)
    assert items[1]["ligand"].pos.is_cuda and torch.equal(items[1]["ligand"].pos, case["got_dev"][2])
    # the raw call: capacity status, nothing launched, nothing written
    lib = engine.load_library()
    edges, bits = pack_ligand(big)
    nl, r = 230, MAX_TORSIONS + 1
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lig_ptr, rot_ptr, mask_ptr = up(np.array([0, nl], np.int32)), up(np.array([0, r], np.int32)), up(np.array([0, bits.size], np.int32))
    pos, e_dev, b_dev = big["ligand"].pos.to(dev), up(edges), up(bits.view(np.int32))
    tr, rot, tor = up_big[0].to(dev), up(up_big[1].astype(np.float32)), up(up_big[2].astype(np.float32))
    out = torch.full((nl, 3), -77.0, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.cbd_noise_conformers(1, nl, r, p(lig_ptr), p(pos), p(rot_ptr), p(e_dev), p(mask_ptr), p(b_dev), p(tr), p(rot), p(tor), p(out),
                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert rc == -4 and b"128" in lib.cbd_last_error()                      # CBD_ERR_CAPACITY
    assert bool((out == -77.0).all())
    assert lib.cbd_noise_conformers(1, 513, 0, p(lig_ptr), p(pos), p(rot_ptr), None, p(mask_ptr), None, p(tr), p(rot), None, p(out), None) == -4
    torch.cuda.synchronize()
    assert bool((out == -77.0).all())


def test_train_step_on_device_noised_items_equals_the_host_fed_step():
    """device-resident `pos` changes nothing downstream: one train_step at batch 3 on items noised by apply_noise_batch, and one on the
    same positions copied to the host and fed the old way -- losses and gradients bitwise equal"""
    from confidence_bootstrapping_amd.synthetic import make_complex
    from confidence_bootstrapping_amd.training import loss_function, train_step
    from confidence_bootstrapping_amd.utils import load_model_args, make_score_model
    dev = torch.device("cuda:0")
    margs = load_model_args()
    t2s = _t_to_sigma()
    kws = [dict(Nl=8, Nr=30, R=1, knn=8, seed=11), dict(Nl=12, Nr=40, R=2, knn=8, seed=12), dict(Nl=10, Nr=36, R=3, knn=8, seed=13)]
    items = [make_complex(name=f"nz{i}", **kw) for i, kw in enumerate(kws)]
    np.random.seed(3)
    torch.manual_seed(3)
    _transform().apply_noise_batch(items, dev)
    assert all(d["ligand"].pos.is_cuda for d in items)
    fed = []
    for d in items:
        h = d.shallow_copy()
        h["ligand"].pos = d["ligand"].pos.cpu()
        fed.append(h)
    loss_fn = partial(loss_function, tr_weight=0.33, rot_weight=0.33, tor_weight=0.33, no_torsion=False)
    runs = []
    for data in (items, fed):
        model, _ = make_score_model(device=dev, seed=0, args=margs, eval_mode=False)
        model.train()
        opt = torch.optim.SGD(model.parameters(), lr=0.0)
        torch.manual_seed(123)
        torch.cuda.manual_seed_all(123)
        out = train_step(model, data, opt, dev, t2s, loss_fn)
        torch.cuda.synchronize()
        assert out is not None
        runs.append(([o.detach().clone() for o in out], {n: (None if p.grad is None else p.grad.clone()) for n, p in model.named_parameters()}))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert bool(torch.isfinite(runs[0][0][0]).all())
    diff = [n for n, g in runs[0][1].items() if (g is None) != (runs[1][1][n] is None) or (g is not None and not torch.equal(g, runs[1][1][n]))]
    assert not diff, diff[:5]
    assert sum(g is not None and bool(g.abs().sum() > 0) for g in runs[0][1].values()) > 10
