"""The a-priori bounds of tests/train_kernel_helpers.py are satisfiable and not vacuous.  For every case of tests/test_gpu_train_kernels.py:
the magnitude companion dominates |ref64|; the same operation by torch in float32 on the CPU (its own fp32 autograd; a sequential fp32
sum for the segmented sums) lies within the bounds against the float64 reference, with the fp32 sum lengths torch really has (E_g for a
weight gradient, N * d for a BatchNorm statistic) -- a correct fp32 implementation passes before any GPU run, and the ratios printed
(pytest -s) are the REFERENCE's own, not the kernels'; a wrong term lies outside the bounds by the stated factor; and the chunk and
kernel-selection rules, as the helpers state them, give the shapes the GPU cases name."""
import math

import pytest
import torch

from tests import train_kernel_helpers as H


# ================================================================================================================ 1. first stage
@pytest.mark.parametrize("sizes", H.FC_LAYOUTS, ids=H.fc_id)
def test_first_stage_torch_fp32_lies_within_the_bounds(sizes):
    case = H.fc_case(sizes)
    pre, ab_pre = H.fc_pre64(sizes)
    E = sum(sizes)
    assert pre.shape == (E, H.FC_K) and H.dominates(ab_pre, pre)
    bound = H.FC_N_HID * H.U * ab_pre + H.FLOOR
    x32, lo, outs = case["x"], 0, []
    for k, n in enumerate(sizes):
        outs.append(torch.relu(torch.nn.functional.linear(x32[lo:lo + n], case["W"][k], case["b"][k])))
        lo += n
    hid32 = torch.cat(outs)
    worst, share = H.fc_check_forward(hid32, pre, bound)
    print(f"first stage torch fp32 vs fp64, {H.fc_id(sizes)}: hid error / bound {worst:.3f}, share inside the sign band {share:.2e}")
    assert worst <= 1
    g = torch.Generator().manual_seed(99)
    for p in H.FC_DROPOUT:
        keep = (torch.rand(E, H.FC_K, generator=g) >= p) & (hid32 > 0)
        M = keep.double() / (1.0 - p)
        ref, ab = H.fc_grads64(case, M)
        for k in ("dW", "db"):
            assert all(H.dominates(a, r) for a, r in zip(ab[k], ref[k])), k
        assert H.dominates(ab["gx"], ref["gx"])
        got = H.fc_grads64(case, keep.float() * H.fc_scale32(p), torch.float32)
        r = H.fc_grad_ratios(got, ref, H.fc_grad_bounds(case, ab, rows=list(sizes)))
        print(f"first stage torch fp32 vs fp64, {H.fc_id(sizes)}, p = {p}: largest error / bound {H.fmt(r)}")
        assert all(v <= 1 for v in r.values()), r


def test_first_stage_a_wrong_term_exceeds_the_bounds():
    """one row dropped from a dW1 chunk: > 1000 times outside the bounds of dW1 and db1; one mask element flipped: > 1000 times outside
    the bound of gx (and outside those of dW1 / db1); the scale 1 / (1 - p) left out of the backward pass: > 1000 times outside"""
    sizes = (2049,)
    case = H.fc_case(sizes)
    pre, _ = H.fc_pre64(sizes)
    M = (pre > 0).double() / 0.75
    ref, ab = H.fc_grads64(case, M)
    bnd = H.fc_grad_bounds(case, ab)
    assert H.fc_parts(2049) == (33, 64)
    short = dict(case, gout=case["gout"].clone())
    short["gout"][100] = 0.0                                              # row 100 takes no part in the sums
    r = H.fc_grad_ratios(H.fc_grads64(short, M)[0] | {"gx": ref["gx"]}, ref, bnd)
    print(f"row dropped: {H.fmt(r)}")
    assert r["dW1"] > 1000 and r["db1"] > 1000
    M2 = M.clone()
    e, j = 7, int(torch.nonzero(M[7] > 0)[0])
    M2[e, j] = 0.0
    r = H.fc_grad_ratios(H.fc_grads64(case, M2)[0], ref, bnd)
    print(f"mask element flipped: {H.fmt(r)}")
    assert r["gx"] > 1000 and r["dW1"] > 1 and r["db1"] > 1
    r = H.fc_grad_ratios(H.fc_grads64(case, M * 0.75)[0], ref, bnd)
    assert min(r.values()) > 1000


def test_first_stage_chunk_rule_gives_the_shapes_the_gpu_cases_name():
    assert H.fc_parts(65537) == (1024, 66)                                 # ceil(65537 / 1024) = 65, rounded up to even
    parts, chunk = H.fc_parts(65537)
    rows = [max(0, min(65537, (k + 1) * chunk) - k * chunk) for k in range(parts)]
    assert sum(rows) == 65537 and all(n == 66 for n in rows[:992]) and rows[992] == 65 and rows[993:] == [0] * 31
    assert 993 * chunk == 65538 > 65537                                    # the empty parts start PAST the group's end (e_lo > E1)
    assert H.fc_parts(2049) == (33, 64) and 2049 - 32 * 64 == 1
    assert [H.fc_parts(n) for n in (1, 31, 32, 33, 65, 511, 512, 513)] == [(1, 2), (1, 32), (1, 32), (1, 34), (2, 34), (8, 64), (8, 64), (9, 58)]
    assert H.FC_ROWS_PER_WG == 512
    assert H.fc_workgroups((512,)) == [1] and H.fc_workgroups((513,)) == [2] and H.fc_workgroups((511, 1, 512)) == [1, 1, 1]
    assert H.fc_workgroups((65537,)) == [129]
    assert max(len(s) for s in H.FC_LAYOUTS) == H.FC_MAX_GROUPS
    assert abs(H.fc_scale32(0.25) - 4.0 / 3.0) < 1e-7 and H.fc_scale32(0.0) == 1.0


# ================================================================================================================ 2. segmented sums
@pytest.mark.parametrize("c", H.SEG_CASES, ids=lambda c: f"N{c[0]}-W{c[1]}")
def test_segment_sums_sequential_fp32_lies_within_the_bounds(c):
    N, W = c
    case = H.seg_case(N, W)
    counts, index = case["counts"], case["index"]
    assert torch.equal(torch.bincount(index, minlength=N), counts) and int(counts.max()) == 4099
    assert N == 1 or sorted(set(H.SEG_SPECIAL)) == sorted(set(H.SEG_SPECIAL) & set(counts.tolist()))
    assert N == 1 or not torch.equal(index, torch.sort(index)[0])                   # the edges are permuted
    ref, ab = H.seg_sum64(case["vals"], index, N)
    assert H.dominates(ab, ref)
    got = H.seg_sum32_sequential(case["vals"], index, N)
    cnt32 = counts.clamp(min=1).float()[:, None]
    r = {"sum": H.ratio(got, ref, H.seg_bounds(counts, ab)),
         "mean": H.ratio(got / cnt32, ref / counts.clamp(min=1)[:, None], H.seg_bounds(counts, ab, mean=True))}
    cnt = counts.clamp(min=1).double()[:, None]
    gb64 = (case["g_rows"].double() / cnt)[index]
    gb32 = (case["g_rows"] * (1.0 / cnt32))[index]
    r["mean bwd"] = H.ratio(gb32, gb64, 2 * H.U * gb64.abs() + H.FLOOR)
    print(f"sequential fp32 vs fp64, N = {N}, W = {W} ({index.numel()} edges): largest error / bound {H.fmt(r)}")
    assert all(v <= 1 for v in r.values()), r


def test_segment_sum_with_one_edge_dropped_exceeds_the_bound():
    """one edge dropped from the run of 4099: the bound of that row is 4101 u sum|v| ~ 0.8 per element, the width of a worst-case fp32 sum
    of 4099 terms, so only an edge with a large value shows: the edge of the hub row with the largest entry lies > 3 times outside;
    the same edge dropped from a run of 17 lies > 10^5 times outside"""
    case = H.seg_case(1025, 80)
    counts, index, vals = case["counts"], case["index"], case["vals"]
    ref, ab = H.seg_sum64(vals, index, 1025)
    bnd = H.seg_bounds(counts, ab)
    for length, factor in ((4099, 3.0), (17, 1e5)):
        row = int(torch.nonzero(counts == length)[0])
        edges = torch.nonzero(index == row)[:, 0]
        e = int(edges[vals[edges].abs().max(1)[0].argmax()])
        v = vals.clone()
        v[e] = 0.0
        r = H.ratio(H.seg_sum64(v, index, 1025)[0], ref, bnd)
        print(f"one edge dropped from a run of {length}: {r:.3g} times the bound")
        assert r > factor


def test_segment_cases_cover_what_the_gpu_file_names():
    assert [H.seg_kernel(n) for n in H.SEG_NS] == ["long16", "long16", "long4", "long4", "wave"]
    for N in H.SEG_NS:
        assert {3, 65, 80} <= {w for n, w in H.SEG_CASES if n == N}
    for W in H.SEG_WIDTHS:
        assert {64, 1025} <= {n for n, w in H.SEG_CASES if w == W}
    assert any(64 < w < 128 for w in H.SEG_WIDTHS) and sum(1 for w in H.SEG_WIDTHS if w % 4) >= 1
    for N, W in H.SEG_CASES:
        assert H.seg_case(N, W)["index"].numel() <= 12000                  # about 10^4 edges


@pytest.mark.parametrize("c", H.EDGE_CAT_CASES, ids=lambda c: f"N{c[0]}-D{c[1]}")
def test_edge_cat_backward_sequential_fp32_lies_within_the_bound(c):
    case = H.edge_cat_case(*c)
    N = c[0]
    ref, ab, bnd = H.edge_cat_ref64(case)
    assert H.dominates(ab, ref) and int(case["cs"].sum()) == int(case["cd"].sum())
    if N > 1:
        assert bool(((case["cs"] > 0) & (case["cd"] == 0)).any()) and bool(((case["cs"] == 0) & (case["cd"] > 0)).any())
    got = H.seg_sum32_sequential(case["g"][:, 32:64], case["src"], N) + H.seg_sum32_sequential(case["g"][:, 64:96], case["dst"], N)
    r = H.ratio(got, ref, bnd)
    print(f"edge_cat backward, sequential fp32 vs fp64, N = {N}: largest error / bound {r:.3f}")
    assert r <= 1


# ================================================================================================================ 3. BatchNorm
BN_CASES = [(lay, N) for lay in H.BN_LAYOUTS for N in H.BN_NS]


@pytest.mark.parametrize("c", BN_CASES, ids=H.bn_id)
def test_batch_norm_torch_fp32_lies_within_the_bounds(c):
    (irreps, ldx, res_dim), N = c
    fields, D = H.bn_fields(irreps)
    dmax = max(d for _, d, _ in fields)
    for regime in H.BN_REGIMES:
        case, ref, ab, pieces = H.bn_reference(irreps, ldx, res_dim, N, regime)
        assert case["x"].shape == (N, ldx) and ldx >= D > res_dim
        for k in ("y", "gx", "gw", "gb", "running_var", "running_mean"):
            assert H.dominates(ab[k], ref[k]), k
        got = H.bn_torch32(case)
        r = H.bn_ratios(got, ref, H.bn_bounds(ab, n_extra=N * dmax))
        print(f"BatchNorm torch fp32 vs fp64, {irreps}, N = {N}, {regime} (n + {N * dmax}): largest error / bound {H.fmt(r)}")
        assert all(v <= 1 for v in r.values()), r


def test_batch_norm_without_the_m0_term_exceeds_the_bound():
    """gx = w r (g - chat m1 - m0): with m0 = mean(g) left out, the 0e columns lie > 1000 times outside the kernels' bound (N = 341: m0 is
    of size 1 / sqrt(341) of g), in both data regimes"""
    irreps, ldx, res_dim = H.BN_LAYOUTS[3]
    for regime in H.BN_REGIMES:
        case, ref, ab, pieces = H.bn_reference(irreps, ldx, res_dim, 341, regime)
        bnd = H.bn_bounds(ab)
        r = H.ratio(ref["gx"] + pieces["m0_term"], ref["gx"], bnd["gx"])
        print(f"m0 left out, {regime}: {r:.3g} times the bound")
        assert r > 1000
        assert float(pieces["m0_term"][:, 32:].abs().max()) == 0.0           # the other fields have no m0


def test_batch_norm_cases_sit_on_the_stride_boundaries():
    assert {1023, 1024, 1025} <= set(H.BN_NS) and 341 * 3 == 1023 and 342 * 3 == 1026          # BN_THREADS = 1024
    assert [H.bn_fields(lay[0])[1] for lay in H.BN_LAYOUTS] == [32, 50, 68, 74, 12]
    assert not any(z for _, _, z in H.bn_fields("2x1o+2x1e")[0])
    for N in H.BN_EXCL_NS:
        for ex in H.bn_excludes(N):
            live = H.bn_live(N, ex)
            assert 0 < int(live.sum()) < N and max(hi for _, hi in ex) <= N
        assert any(hi == N for ex in H.bn_excludes(N) for _, hi in ex)
    # the reference over the live rows alone: the shapes follow the live rows
    case = H.bn_case(*H.BN_LAYOUTS[1], 342, "unit")
    live = H.bn_live(342, H.bn_excludes(342)[0])
    ref, ab, _ = H.bn_ref64(case, live)
    assert ref["y"].shape == (342 - 22, 50) and ref["gw"].shape == (38,) and ref["gb"].shape == (32,)


# ================================================================================================================ 4. heads
@pytest.mark.parametrize("c", H.CENTER_CASES, ids=H.head_id)
def test_centre_head_torch_fp32_lies_within_the_bounds(c):
    case, ref, ab = H.center_reference(c)
    n = c[0]
    assert ref["out"].shape == (n, 12) and ref["gx"].shape == (n, c[1]) and ref["gw"].shape == (n, 124)
    assert float(ref["gx"][:, H.HEAD_DIM:].abs().sum()) == 0.0
    # the restatement the companion is built from is the package's formula
    v = H._unit64(case["vec"], math.sqrt(3.0))
    assert torch.allclose(H.center_form(case["x"].double(), v, case["w"].double()), ref["out"], rtol=1e-12, atol=1e-300)
    for k in ("out", "gx", "gw"):
        assert H.dominates(ab[k], ref[k]), k
    r = H.head_ratios(H.center_eval(case, torch.float32), ref, H.center_bounds(ab))
    print(f"centre head torch fp32 vs fp64, {H.head_id(c)}: largest error / bound {H.fmt(r)}")
    assert all(v <= 1 for v in r.values()), r


@pytest.mark.parametrize("c", H.BOND_CASES, ids=H.head_id)
def test_bond_head_torch_fp32_lies_within_the_bounds(c):
    case, ref, ab = H.bond_reference(c)
    n = c[0]
    assert ref["out"].shape == (n, 64) and ref["gx"].shape == (n, c[1]) and ref["gw"].shape == (n, 384)
    assert float(ref["gx"][:, :32].abs().sum()) == 0.0 and float(ref["gx"][:, 68:].abs().sum()) == 0.0
    v, b = H._unit64(case["evec"], math.sqrt(3.0)), H._unit64(case["bvec"], 1.0)
    assert torch.allclose(H.bond_form(case["x"].double(), v, b, case["w"].double()), ref["out"], rtol=1e-12, atol=1e-300)
    for k in ("out", "gx", "gw"):
        assert H.dominates(ab[k], ref[k]), k
    r = H.head_ratios(H.bond_eval(case, torch.float32), ref, H.bond_bounds(ab))
    print(f"bond head torch fp32 vs fp64, {H.head_id(c)}: largest error / bound {H.fmt(r)}")
    assert all(v <= 1 for v in r.values()), r


def test_head_special_rows_are_what_the_cases_name():
    case = H.center_case(65, 80, None)
    nrm = case["vec"].double().norm(dim=1)
    assert float(nrm[0]) == 0.0 and 0 < float(nrm[1]) < 1e-12 and abs(float(nrm[2]) - 1e3) < 1e-2
    # below F.normalize's eps both precisions take the same branch: v = p / 1e-12
    assert torch.allclose(torch.nn.functional.normalize(case["vec"][1:2], dim=-1).double(), case["vec"][1:2].double() / 1e-12, rtol=1e-6)
    case = H.bond_case(65, 74, None)
    e, b = case["evec"].double(), case["bvec"].double()
    assert float(torch.linalg.cross(e[3], b[3]).norm()) <= 1e-6 * float(e[3].norm() * b[3].norm()) and float(e[3].norm()) > 0
    assert float(H.bond_case(1, 74, 3)["evec"][0].norm()) > 0 and float(H.center_case(1, 74, 0)["vec"][0].norm()) == 0.0
    assert {c[0] for c in H.CENTER_CASES} == {1, 63, 64, 65, 129} and {c[0] for c in H.BOND_CASES} == {1, 2, 3, 65}
    assert {c[1] for c in H.CENTER_CASES} == {74, 80} == {c[1] for c in H.BOND_CASES}


def test_centre_head_without_one_inverse_sqrt2_exceeds_the_bound():
    """the 1 / sqrt2 of the 1e x 1o -> 1o path left out: the 1o outputs lie > 1000 times outside their bound, the 1e outputs unchanged"""
    c = (65, 80, None)
    case, ref, ab = H.center_reference(c)
    v = H._unit64(case["vec"], math.sqrt(3.0))
    wrong = H.center_form(case["x"].double(), v, case["w"].double(), s2e=1.0)
    bnd = H.center_bounds(ab)["out"]
    r = H.ratio(wrong[:, :6], ref["out"][:, :6], bnd[:, :6])
    print(f"1 / sqrt2 left out: {r:.3g} times the bound")
    assert r > 1000 and torch.equal(wrong[:, 6:], H.center_form(case["x"].double(), v, case["w"].double())[:, 6:])
