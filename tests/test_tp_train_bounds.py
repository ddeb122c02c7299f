"""The a-priori bounds of tests/tp_train_helpers.py are satisfiable: for every case of tests/test_gpu_tp_train.py the oracle formula
evaluated by torch in float32 on the CPU, with torch's own fp32 autograd, lies within the bounds against tp_ref64 -- a correct fp32
implementation passes before any GPU run.  The weight / bias gradient bound uses n = E_g + 11 here: torch sums all edges of a group in
fp32.  The ratios printed are the REFERENCE's own (pytest -s shows them), not the kernels'.  Also: tp_abs64 >= |tp_ref64| elementwise,
and the shapes the GPU cases rely on follow from the chunk rule as the helpers state it."""
import pytest
import torch

from tests import tp_train_helpers as H


def _flat(r):
    return [("msg", r["msg"]), ("gx", r["gx"]), ("gh", r["gh"])] + [(f"dW2[{g}]", t) for g, t in enumerate(r["dW2"])] + \
           [(f"db2[{g}]", t) for g, t in enumerate(r["db2"])]


@pytest.mark.parametrize("c", H.ALL_CASES, ids=H.case_id)
def test_torch_fp32_lies_within_the_bounds(c):
    IN, OUT, groups = c
    case, ref, ab = H.reference(IN, OUT, groups, H.seed_of(*c))
    d = H.dims(IN, OUT)
    assert ref["msg"].shape == (sum(groups), d["out_dim"]) and ref["gx"].shape == (sum(groups), d["in_dim"])
    assert case["W2"][0].shape == (d["W"], H.KDIM)
    assert int((case["h"] == 0).sum()) > 0 or sum(groups) == 0
    # the companion dominates the reference (1e-12: both are fp64 sums of the same terms in different orders)
    for (name, a), (_, r) in zip(_flat(ab), _flat(ref)):
        assert a.shape == r.shape and bool((a * (1 + 1e-12) + H.FLOOR >= r.abs()).all()), name
    for g, n in enumerate(groups):
        if n:
            assert bool((ab["gw"][g] * (1 + 1e-12) + H.FLOOR >= ref["gw"][g].abs()).all())
            # what test d compares with: dW2 = g_w^T h, db2 = column sums of g_w
            lo = sum(groups[:g])
            assert torch.allclose(ref["gw"][g].t() @ case["h"][lo:lo + n].double(), ref["dW2"][g], rtol=1e-12, atol=1e-300)
            assert torch.allclose(ref["gw"][g].sum(0), ref["db2"][g], rtol=1e-12, atol=1e-300)
        else:
            assert float(ref["dW2"][g].abs().max()) == 0.0 and float(ref["db2"][g].abs().max()) == 0.0
    got = H.tp_torch32(case)
    bnd = H.bounds(case, ab, dw_edges=list(groups))
    r = H.ratios(got, ref, bnd)
    print(f"torch fp32 (the reference's own) vs fp64, {H.case_id(c)}: largest error / bound {H.fmt(r)}")
    assert all(v <= 1 for v in r.values()), r


def test_a_wrong_term_exceeds_the_bounds():
    """the bounds are not vacuous: one edge's contribution dropped from the weight gradient is a hundred times outside them, and so
    is a relative error of 1e-4 in a message or of 1e-2 in g_h (a chain of wp = 1728 terms that largely cancel: the loosest bound)"""
    c = (3, 3, (65,))
    case, ref, ab = H.reference(*c, H.seed_of(*c))
    bnd = H.bounds(case, ab)
    short = H.slice_case(case, 0)
    for k in ("x", "vec", "h", "gout"):
        short[k] = short[k][:64]
    short["groups"] = (64,)
    r64 = H.tp_ref64(short)
    assert H.ratio(r64["dW2"][0], ref["dW2"][0], bnd["dW2"][0]) > 100 and H.ratio(r64["db2"][0], ref["db2"][0], bnd["db2"][0]) > 100
    assert H.ratio(ref["msg"] * (1 + 1e-4), ref["msg"], bnd["msg"]) > 1 and H.ratio(ref["gh"] * (1 + 1e-2), ref["gh"], bnd["gh"]) > 1


def test_chunk_rule_gives_the_shapes_the_gpu_cases_name():
    assert [H.dims(i, o)["wp"] for i, o in H.LEVELS] == [1248, 1536, 1664, 1728]
    assert [H.dims(i, o)["W"] for i, o in H.LEVELS] == [1216, 1480, 1588, 1660]
    assert [-(-(H.dims(i, o)["wp"] // 32) // 4) for i, o in H.LEVELS] == [10, 12, 13, 14]          # grid.x of tp_train_dw_kernel
    assert H.dw_chunks(1153) == (9, 5) and 37 - 7 * 5 == 2 and 37 - 8 * 5 < 0
    assert H.dw_chunks(2145) == (17, 4) and 2145 - 67 * 32 == 1
    assert [H.dw_chunks(n)[0] for n in (1153, 300, 33)] == [9, 2, 1]
    assert H.dw_chunks(600, cap=3) == (3, 7) and 19 - 2 * 7 == 5
    assert H.dw_chunks(2000) == (15, 5) and H.dw_chunks(65) == (1, 3) and H.dw_chunks(1) == (1, 1)
