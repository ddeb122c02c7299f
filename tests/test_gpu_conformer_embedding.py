"""Conformer embedding on the GPU (csrc/conformer_embed.hip through datasets/conformer_embedding.py) against the float64 restatement
of the acceptance test in tests/embed_helpers.py, which is written from the bounds and never calls the kernel.

One launch embeds 32 conformers of each of the seven test molecules (4 .. 65 atoms; 65 = a second 64-lane stride); the tests share it.
Measured on an MI355X (seed 0): 32 of 32 first attempts ok for every molecule (the floor the test sets is 24); the worst distance
excess of an ok conformer 0.002 A (1a0q); cyclohexane's ring atoms 0.23 .. 0.39 A (rms) off their plane, benzene's 0.0000 A; 1a0q end
to end: rmsd_matching 0.216 A after torsion matching against 2.248 A aligned only.  DESIGN.md section 9 records the same figures."""
import numpy as np
import pytest
import torch

from tests import embed_helpers as eh

pytestmark = pytest.mark.gpu
N_CONF = 32
BAND = 1e-3          # relative: the band around every limit in which the kernel's fp32 evaluation may decide either way


@pytest.fixture(scope="module")
def world():
    from confidence_bootstrapping_amd.datasets import conformer_embedding as ce
    mols = eh.molecules()
    names = list(mols)
    bounds = {k: ce.distance_bounds(m, ref) for k, (m, ref) in mols.items()}
    res = ce.embed_conformers_batch([bounds[k] for k in names], N_CONF, seed=0)          # seven molecules, one launch
    return {"mols": mols, "names": names, "bounds": bounds, "res": dict(zip(names, res))}


def _best_plane_rms(p):
    q = p - p.mean(0)
    return float(np.linalg.svd(q, compute_uv=False)[-1] / np.sqrt(len(p))), float(np.abs(q @ np.linalg.svd(q)[2][-1]).max())


def test_acceptance(world):
    from confidence_bootstrapping_amd.datasets import conformer_embedding as ce
    for name in world["names"]:
        lower, upper, cons = world["bounds"][name]
        pos, ok, err = world["res"][name]
        assert pos.shape == (N_CONF, len(lower), 3) and np.isfinite(pos).all() and np.isfinite(err).all()
        for k in range(N_CONF):
            if ok[k]:
                assert eh.accepted(pos[k], lower, upper, cons, ce.BOUND_TOL, widen=BAND), (name, k, eh.violations(pos[k], lower, upper, cons))
            else:
                assert not eh.accepted(pos[k], lower, upper, cons, ce.BOUND_TOL, widen=-BAND), (name, k)
        worst = max((eh.violations(pos[k], lower, upper, cons)[0] for k in range(N_CONF) if ok[k]), default=float("nan"))
        print(f"{name}: {int(ok.sum())} of {N_CONF} first attempts ok; worst distance excess of an ok conformer {worst:.4f} A; "
              f"median error {np.median(err):.2e}")
        assert ok.sum() >= 24, (name, int(ok.sum()))


def test_handedness_pucker_and_planarity(world):
    from confidence_bootstrapping_amd.datasets import conformer_embedding as ce
    signs = {}
    for name in ("chiral_r", "chiral_s"):
        mol, ref = world["mols"][name]
        pos, ok, _ = world["res"][name]
        want = np.sign(ce.centre_volume(ref, (0, 1, 2, 3)))
        got = np.array([np.sign(ce.centre_volume(p, (0, 1, 2, 3))) for p in pos[ok]])
        assert len(got) and (got == want).all(), name
        signs[name] = want
    assert signs["chiral_r"] == -signs["chiral_s"]
    # the stereo-centre of the ligand (C0: P, N, C) keeps the crystal's hand
    mol, ref = world["mols"]["1a0q"]
    pos, ok, _ = world["res"]["1a0q"]
    assert all(np.sign(ce.centre_volume(p, (0, 22, 21, 1))) == np.sign(ce.centre_volume(ref, (0, 22, 21, 1))) for p in pos[ok])
    # cyclohexane: a chair's ring atoms lie 0.23 A off their mean plane; under half of that counts as flattened
    pos, ok, _ = world["res"]["cyclohexane"]
    flat = [_best_plane_rms(p[:6])[0] for p in pos[ok]]
    print(f"cyclohexane: rms distance of the ring atoms from their plane {min(flat):.3f} .. {max(flat):.3f} A")
    assert min(flat) > 0.1
    pos, ok, _ = world["res"]["benzene"]
    off = [_best_plane_rms(p)[1] for p in pos[ok]]
    print(f"benzene: largest distance of a ring atom from the ring plane {max(off):.4f} A")
    assert max(off) <= ce.PLANAR_LIMIT


def test_repeatable_and_independent_of_the_launch(world):
    from confidence_bootstrapping_amd.datasets import conformer_embedding as ce
    for m, name in enumerate(world["names"]):
        if name not in ("chain4", "1a0q", "alkane65"):
            continue
        b = world["bounds"][name]
        pos, ok, err = world["res"][name]
        alone = ce.embed_conformers_batch([b], N_CONF, seed=0, mol_ids=[m])[0]                  # the 32 without the other molecules
        assert np.array_equal(alone[0], pos) and np.array_equal(alone[1], ok) and np.array_equal(alone[2], err), name
        one = ce.embed_conformers_batch([b], 1, seed=0, mol_ids=[m], conf_ids=[[5]])[0]          # one conformer on its own
        assert np.array_equal(one[0][0], pos[5]) and one[1][0] == ok[5] and one[2][0] == err[5], name
        other = ce.embed_conformers_batch([b], 2, seed=1, mol_ids=[m])[0]
        assert not np.array_equal(other[0][0], pos[0]) and not np.array_equal(other[0][0], other[0][1]), name


def test_capacity_and_bad_indices_write_nothing(world):
    import ctypes as C
    from confidence_bootstrapping_amd import engine
    from confidence_bootstrapping_amd.datasets import conformer_embedding as ce
    lower, upper, cons = world["bounds"]["chiral_r"]
    bad = dict(cons, idx=cons["idx"].copy())
    bad["idx"][0, 3] = 5                                          # 5 atoms: index 5 is outside
    with pytest.raises(ValueError):
        ce.embed_conformers_batch([(lower, upper, bad)], 1)
    with pytest.raises(ValueError):
        ce.embed_conformers_batch([(np.zeros((257, 257)), np.ones((257, 257)), dict(cons, idx=cons["idx"][:0], lo=[], hi=[], kind=[]))], 1)
    # the C ABI without the Python checks in front of it; every size stays inside the buffers
    lib = engine.load_library()
    dev = torch.device("cuda")
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    n = 5
    lo_d, up_d = torch.tensor(lower, dtype=torch.float32, device=dev), torch.tensor(upper, dtype=torch.float32, device=dev)
    idx, kind = i32(bad["idx"]), i32(cons["kind"])
    clo, chi = torch.tensor(cons["lo"], dtype=torch.float32, device=dev), torch.tensor(cons["hi"], dtype=torch.float32, device=dev)
    mol_n, bnd_ptr, cons_ptr = i32([n]), i32([0, n * n]), i32([0, len(kind)])
    conf_mol, conf_id, out_ptr = i32([0]), i32([0]), i32([0, n])
    pos = torch.full((n, 3), 7.0, device=dev)
    err, ok = torch.full((1,), 7.0, device=dev), i32([7])
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(max_n, max_cons):
        rc = lib.cbd_embed_conformers(1, 1, max_n, max_cons, p(mol_n), p(bnd_ptr), p(lo_d), p(up_d), p(cons_ptr), p(idx), p(clo), p(chi), p(kind),
                                      None, p(conf_mol), p(conf_id), p(out_ptr), 0, 10, 10, 10, 0.05, p(pos), p(err), p(ok), None)
        torch.cuda.synchronize()
        return rc

    assert call(257, len(kind)) == -4 and call(n, 1025) == -4                  # capacity: CBD_ERR_CAPACITY, no launch
    assert (pos == 7.0).all() and err.item() == 7.0 and ok.item() == 7
    assert call(n, len(kind)) == 0                                             # the out-of-range constraint index: refused on the device
    assert (pos == 7.0).all() and np.isnan(err.item()) and ok.item() == -1
    idx.copy_(i32(cons["idx"]))
    assert call(n, len(kind)) == 0 and ok.item() in (0, 1) and not (pos == 7.0).any()       # the same call with the index in range


def test_end_to_end_ligand_graph(world):
    from confidence_bootstrapping_amd.datasets import process_mols as pm, conformer_embedding as ce, conformer_matching as cm
    from confidence_bootstrapping_amd.hetero import HeteroData
    read = lambda: pm.read_molecule(eh.SDF_1A0Q, sanitize=True)
    plain = HeteroData()
    pm.get_lig_graph_with_matching(read(), plain, matching=False, keep_original=True, remove_hs=True)
    g = HeteroData()
    kept = pm.get_lig_graph_with_matching(read(), g, matching=True, conformers="embed", keep_original=True, remove_hs=True, popsize=15, maxiter=30)
    assert torch.equal(g["ligand"].x, plain["ligand"].x)
    assert torch.equal(g["ligand", "lig_bond", "ligand"].edge_index, plain["ligand", "lig_bond", "ligand"].edge_index)
    assert torch.equal(g["ligand"].edge_mask, plain["ligand"].edge_mask)
    holo = np.asarray(plain["ligand"].orig_pos)
    assert np.array_equal(np.asarray(g["ligand"].orig_pos), holo)
    lower, upper, cons = world["bounds"]["1a0q"]
    pose = g["ligand"].pos.numpy().astype(np.float64)
    print("kept pose: violations (distance, volume, planarity) =", eh.violations(pose, lower, upper, cons))
    assert eh.accepted(pose, lower, upper, cons, ce.BOUND_TOL)
    g2 = HeteroData()
    pm.get_lig_graph_with_matching(read(), g2, matching=True, conformers="embed", skip_matching=True, remove_hs=True)
    print(f"1a0q: rmsd_matching {g.rmsd_matching:.4f} A after torsion matching, {g2.rmsd_matching:.4f} A aligned only")
    assert np.isfinite(g.rmsd_matching) and g.rmsd_matching <= g2.rmsd_matching
    mol = eh.ligand_1a0q()
    assert pm.generate_conformer(mol, seed=0) is False
    new = mol.GetConformer().GetPositions()
    assert not np.allclose(new, holo) and eh.accepted(new, lower, upper, cons, ce.BOUND_TOL, widen=BAND)
