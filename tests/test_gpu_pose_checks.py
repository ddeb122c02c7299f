"""cbd_pose_checks (csrc/pose_checks.hip) through evaluation.pose_checks_batch: ONE ragged launch over the cases of
tests/pose_check_helpers.py -- ligands of 1, 2, 63, 64, 65 and 256 atoms (no pair; the pair loop below, at and past one wave's and the
workgroup's stride; the capacity), receptors of 0, 1, 255, 256, 257 and 1000 atoms (none; fewer atoms than threads; the tail of the strided
loop), 1 and 3 poses, a receptor shared by two complexes, a complex without tables, a NaN coordinate, a non-positive lower bound, exact
ties across a thread's own stride, across waves and across lanes, and one case per check that fails alone.

The inputs lie on a grid (see the helpers): no pair is within a relative 1e-5 of a threshold and the closest receptor pair is unique or an
exact tie -- asserted on the fp64 brute force before any device result is looked at -- so counts, flags and atoms are compared EXACTLY.  The
floats are compared to within one fp32 step, a derived bound: both sides evaluate the same fp64 expression on the same fp32 inputs to
within a few 2^-53 and round once; fused multiply-adds may differ between them."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.pose_check_helpers import FLOATS, INTS, assert_same, bitwise_equal, brute_checks, expected, gpu_cases, line_case, random_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CBD_ERR_ARG, CBD_ERR_CAPACITY = -1, -4
FILL = 12345
ROWS = FLOATS + INTS          # the rows of the kernel's output, in order


@pytest.fixture(scope="module")
def case():
    from confidence_bootstrapping_amd.evaluation import pose_checks_batch
    dev = torch.device("cuda:0")
    cases = gpu_cases()
    want = expected(cases)          # margins asserted in there, before anything runs on the device
    items = [(c["lp"], c["tables"], c["receptor"]) for c in cases]
    got = pose_checks_batch(items, dev)
    again = pose_checks_batch(items, dev)
    return dict(dev=dev, cases=cases, want=want, items=items, got=got, again=again)


def test_one_ragged_launch_equals_the_brute_force(case):
    from confidence_bootstrapping_amd.evaluation import _pack_pose_checks, _prepare_check_items
    pk = _pack_pose_checks(_prepare_check_items(case["items"]))
    names = [c["name"] for c in case["cases"]]
    assert pk["cplx_rec"][names.index("shared_a")] == pk["cplx_rec"][names.index("shared_b")] >= 0          # one upload for both
    assert {1, 2, 63, 64, 65, 256} <= set(pk["cplx_n"].tolist()) and {1, 3} <= {len(c["lp"]) for c in case["cases"]}
    assert {0, 1, 255, 256, 257, 1000} <= {0 if c["receptor"] is None else len(c["receptor"][0]) for c in case["cases"]}
    for c, got, want in zip(case["cases"], case["got"], case["want"]):
        print(c["name"], "flags", got.flags.tolist(), "rec_ratio", got.rec_ratio.tolist(), "closest", got.rec_lig_atom.tolist(), got.rec_atom.tolist())
        assert_same(got, want, c["name"])
    by = dict(zip(names, case["got"]))
    assert by["n1_a1000"].bond_lo[0] == np.inf and by["n1_a1000"].bond_hi[0] == -np.inf and by["n1_a1000"].n_internal_clash[0] == 0
    assert (by["tie_rec_256_apart"].rec_atom[0], by["tie_rec_64_apart"].rec_atom[0], by["tie_rec_1_apart"].rec_atom[0]) == (44, 71, 199)
    assert (by["tie_lig_pair"].rec_lig_atom[0], by["tie_cross_lanes"].rec_lig_atom[0], by["tie_cross_lanes"].rec_atom[0]) == (2, 1, 300)
    assert [by[n].flags[0] for n in ("all_pass", "bad_bond_only", "bad_angle_only", "internal_clash_only", "rec_clash_only")] == [0, 1, 2, 4, 8]


def test_again_and_alone_bitwise(case):
    from confidence_bootstrapping_amd.evaluation import pose_checks_batch
    for c, a, b in zip(case["cases"], case["got"], case["again"]):
        assert bitwise_equal(a, b), c["name"]
    for c, item, got in zip(case["cases"], case["items"], case["got"]):
        if c["name"] in ("n64_a255", "n256_a1000", "shared_b", "nan_pose", "tie_cross_one_thread", "n256_a0"):
            alone = pose_checks_batch([item], case["dev"])[0]
            assert bitwise_equal(alone, got), c["name"]
    # one pose of a complex launched alone: what it gave among its siblings
    k = [c["name"] for c in case["cases"]].index("n64_a255")
    lp, tables, rec = case["items"][k]
    single = pose_checks_batch([(lp[1:2], tables, rec)], case["dev"])[0]
    assert all(np.array_equal(getattr(single, f).view(np.int32), getattr(case["got"][k], f)[1:2].view(np.int32)) for f in ROWS)


def test_over_capacity_takes_the_host_route_and_thresholds_reach_the_kernel(case):
    from confidence_bootstrapping_amd.evaluation import pose_checks_batch
    big = random_case("n257_a30", 41, 257, 30, 1)
    want, margin, gap = brute_checks(big["lp"], big["tables"], big["receptor"])
    assert margin > 1e-5 and gap > 1e-6
    k = [c["name"] for c in case["cases"]].index("n63_a256")
    got = pose_checks_batch([case["items"][k], (big["lp"], big["tables"], big["receptor"]), (np.zeros((0, 4, 3), np.float32), None, None)], case["dev"])
    assert_same(got[1], want, "n257")
    assert len(got[2].valid) == 0 and bitwise_equal(got[0], case["got"][k])
    loose = line_case("loose", bond=(0, 1, 2.625, 2.875))
    got = pose_checks_batch([(loose["lp"], loose["tables"], loose["receptor"])], case["dev"], bond_tol=0.5)[0]
    assert got.n_bad_bond.tolist() == [0] and got.valid.tolist() == [True]
    assert_same(got, brute_checks(loose["lp"], loose["tables"], loose["receptor"], bond_tol=0.5)[0], "loose")


def _raw(lib, dev, pk, max_n=None, n_poses=None, thresholds=(0.25, 0.25, 0.30, 0.75)):
    """cbd_pose_checks on packed arrays given as they are -> (rc, out int32 [14, P], tail): the output pre-filled with FILL, and 16 words
    behind it that nobody may write"""
    t = lambda a: None if a is None or np.size(a) == 0 else torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    P = len(pk["pose_cplx"]) if n_poses is None else n_poses
    keep = [t(pk[k]) for k in ("pose_cplx", "pose_ptr", "pos", "lig_radius", "cplx_n", "cplx_rec", "cplx_tab", "tab_ptr", "bounds", "kind_words",
                               "rec_ptr", "rec")]
    out = torch.full((14 * len(pk["pose_cplx"]) + 16,), FILL, dtype=torch.int32, device=dev)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    rc = lib.cbd_pose_checks(P, len(pk["cplx_n"]), int(pk["n_receptors"]), int(pk["max_n"]) if max_n is None else max_n, *[p(x) for x in keep],
                             *[C.c_float(v) for v in thresholds], p(out), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    got = out.cpu().numpy()
    return rc, got[:-16].reshape(14, -1), got[-16:]


def _refused(out, p):
    return np.isnan(out[:7, p].view(np.float32)).all() and (out[7:13, p] == -1).all() and out[13, p] == 64


def test_a_contradictory_description_is_refused_without_indexing(case):
    """Invalid input that the kernel must refuse BEFORE it indexes with it: none of these makes it read out of bounds (the altered values
    are never used as an index or an extent)."""
    from confidence_bootstrapping_amd import engine
    from confidence_bootstrapping_amd.evaluation import _pack_pose_checks, _prepare_check_items
    dev, lib = case["dev"], engine.load_library()
    cs = [line_case("all_pass"), line_case("rec_clash_only", rec_atom=[1.5, 2.0, 1.0]), random_case("n9", 51, 9, 40, 3),
          line_case("bad_bond_only", bond=(0, 1, 2.625, 2.875)), line_case("internal_clash_only", other=(0, 3, 7.0, 50.0)),
          line_case("bad_angle_only", angle=(1, 3, 1.625, 2.125))]
    pk = _pack_pose_checks(_prepare_check_items([(c["lp"], c["tables"], c["receptor"]) for c in cs]))
    P = len(pk["pose_cplx"])
    assert P == 8 and pk["n_receptors"] == 6
    rc, clean, tail = _raw(lib, dev, pk)
    assert rc == 0, lib.cbd_last_error().decode()
    assert (tail == FILL).all() and not (clean == FILL).any()
    want = [brute_checks(c["lp"], c["tables"], c["receptor"])[0] for c in cs]
    for k, name in enumerate(ROWS):
        flat = np.concatenate([w[name] for w in want])
        row = clean[k].view(np.float32) if k < 7 else clean[k]
        if k < 7:
            steps = np.abs(row.view(np.int32).astype(np.int64) - flat.view(np.int32).astype(np.int64))
            assert steps.max() <= 1, name
        else:
            assert np.array_equal(row, flat), name
    # pose 0 names no complex; the last pose's extent contradicts cplx_n; complex 3 (pose 5) names no receptor
    bad = {k: np.copy(v) if isinstance(v, np.ndarray) else v for k, v in pk.items()}
    bad["pose_cplx"][0] = len(cs)
    bad["pose_ptr"][P] -= 1
    bad["cplx_rec"][3] = pk["n_receptors"]
    rc, out, tail = _raw(lib, dev, bad)
    assert rc == 0, lib.cbd_last_error().decode()
    print("flags", out[13].tolist())
    assert (tail == FILL).all() and not (out == FILL).any()
    for p in range(P):
        if p in (0, 5, P - 1):
            assert _refused(out, p), p
        else:
            assert np.array_equal(out[:, p], clean[:, p]), p          # the neighbours are not affected
    # the other side of each range, and a table flag that is neither 0 nor 1
    bad = {k: np.copy(v) if isinstance(v, np.ndarray) else v for k, v in pk.items()}
    bad["pose_cplx"][1] = -1
    bad["cplx_rec"][4] = -2
    bad["cplx_tab"][5] = 2
    bad["cplx_n"][0] = 5          # poses of four atoms
    rc, out, tail = _raw(lib, dev, bad)
    assert rc == 0 and (tail == FILL).all() and not (out == FILL).any()
    assert all(_refused(out, p) for p in (0, 1, 6, 7)) and all(np.array_equal(out[:, p], clean[:, p]) for p in (2, 3, 4, 5))


def test_capacity_and_argument_codes_leave_the_outputs_untouched(case):
    from confidence_bootstrapping_amd import engine
    from confidence_bootstrapping_amd.evaluation import _pack_pose_checks, _prepare_check_items
    dev, lib = case["dev"], engine.load_library()
    c = line_case("all_pass")
    pk = _pack_pose_checks(_prepare_check_items([(c["lp"], c["tables"], c["receptor"])]))
    rc, out, tail = _raw(lib, dev, pk, max_n=257)
    assert rc == CBD_ERR_CAPACITY and "257" in lib.cbd_last_error().decode() and (out == FILL).all() and (tail == FILL).all()
    rc, out, tail = _raw(lib, dev, pk, n_poses=0)
    assert rc == 0 and (out == FILL).all() and (tail == FILL).all()          # nothing to do, nothing launched
    assert lib.cbd_pose_checks(0, 0, 0, 0, *([None] * 12), *[C.c_float(v) for v in (0.25, 0.25, 0.3, 0.75)], None, None) == 0
    rc, out, _ = _raw(lib, dev, pk, n_poses=-1)
    assert rc == CBD_ERR_ARG and (out == FILL).all()
    rc, out, _ = _raw(lib, dev, pk, thresholds=(0.25, 0.25, 1.5, 0.75))
    assert rc == CBD_ERR_ARG and (out == FILL).all()
    missing = dict(pk, pos=None)
    rc, out, _ = _raw(lib, dev, missing)
    assert rc == CBD_ERR_ARG and "null" in lib.cbd_last_error().decode() and (out == FILL).all()


def test_dock_front_door_writes_the_checks_and_nothing_else_changes(tmp_path):
    import gzip
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    from confidence_bootstrapping_amd.evaluation import ligand_check_tables, pose_checks, receptor_check_atoms
    from tools import dock
    D = os.path.join(HERE, "golden", "1a0q")
    base = ["--protein", os.path.join(D, "1a0q_protein_processed.pdb.gz"), "--ligand", os.path.join(D, "1a0q_ligand.sdf"), "--samples", "8",
            "--steps", "4"]
    plain, checked = str(tmp_path / "plain"), str(tmp_path / "checked")
    dock.main(base + ["--out", plain])
    dock.main(base + ["--out", checked, "--check-poses"])
    tree = lambda d: {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}
    before, after = tree(plain), tree(checked)
    assert sorted(set(after) - set(before)) == ["pose_checks.csv"]
    assert {k: v for k, v in after.items() if k != "pose_checks.csv"} == before          # file names and ranking: bitwise unchanged
    rows = [r.split(",") for r in after["pose_checks.csv"].decode().splitlines()]
    assert rows[0][:3] == ["rank", "confidence", "valid"] and len(rows) == 1 + 8 and [int(r[0]) for r in rows[1:]] == list(range(1, 9))
    ranked = sorted((f for f in after if f.startswith("rank") and "_confidence" in f), key=lambda f: int(f[4:f.index("_")]))
    written = np.stack([pm.read_molecule(os.path.join(checked, f)).pos for f in ranked]).astype(np.float32)
    pdb = str(tmp_path / "protein.pdb")
    with gzip.open(os.path.join(D, "1a0q_protein_processed.pdb.gz"), "rb") as src, open(pdb, "wb") as dst:
        dst.write(src.read())
    graph = pm.get_receptor(pdb, "1a0q", torch.device("cuda:0"))
    rec = receptor_check_atoms(graph)
    rec = (rec[0] + graph.original_center.cpu().numpy().astype(np.float32), rec[1])
    tables = ligand_check_tables(pm.read_molecule(os.path.join(D, "1a0q_ligand.sdf"), sanitize=True, remove_hs=True))
    want = pose_checks(written, tables, rec)
    print("valid", [r[2] for r in rows[1:]], "flags", [r[16] for r in rows[1:]], "host on the written poses", want.valid.astype(int).tolist())
    assert [int(r[2]) for r in rows[1:]] == want.valid.astype(int).tolist()
    assert [int(r[16]) & (16 | 32 | 64 | 128) for r in rows[1:]] == [0] * 8          # both halves ran
