"""The tensor-product training kernels on the PRODUCTION path (train_ops.StreamHub + train_ops.TensorProductHubFn: tp_train_fwd_kernel,
tp_train_bwd_kernel with gw = NULL, tp_train_gh_kernel, tp_train_dw_kernel of csrc/tp_train.hip and partial_reduce_kernel of
csrc/train_fc.hip) against the float64 oracle of one layer call, within a-priori fp32 bounds per element -- the references, the
counts n behind the bounds, the seeded inputs and the runners are in tests/tp_train_helpers.py; tests/test_tp_train_bounds.py shows on
the CPU that torch's own fp32 arithmetic meets the same bounds for every case here.  Every run is made twice and must repeat bit for
bit.  Every test prints its largest error / bound ratios (pytest -s shows them) before it asserts."""
import pytest
import torch

from tests import tp_train_helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _check(c, got, cap=H.DW_CAP, what="hub"):
    case, ref, ab = H.reference(*c, H.seed_of(*c))
    d = H.dims(c[0], c[1])
    r = H.ratios(got, ref, H.bounds(case, ab, cap=cap))
    print(f"tp train {what} vs fp64, {H.case_id(c)}: largest error / bound {H.fmt(r)}")
    assert all(v <= 1 for v in r.values()), r
    assert got["msg"].shape == (sum(c[2]), H.NODE_STRIDE) and got["gx"].shape == (sum(c[2]), H.NODE_STRIDE)
    assert float(got["msg"][:, d["out_dim"]:].abs().sum()) == 0.0            # padding columns of the messages: exact zeros
    assert float(got["gx"][:, d["in_dim"]:].abs().sum()) == 0.0              # and of the row gradient
    for g, n in enumerate(c[2]):
        if n == 0:                                                           # a group without edges: exactly zero, not garbage
            assert float(got["dW2"][g].abs().max()) == 0.0 and float(got["db2"][g].abs().max()) == 0.0
    return r


@pytest.mark.parametrize("c", H.RAGGED, ids=H.case_id)
def test_ragged_single_group(c):
    """a. One group of E in {1, 31, 32, 33, 65} edges at the four level pairs: below, at and just past one 32-edge wave, a third wave of one
    edge.  msg, x.grad, h.grad, fc[3].weight.grad and fc[3].bias.grad within bounds; the padding columns exactly zero."""
    case, _, _ = H.reference(*c, H.seed_of(*c))
    _check(c, H.run_hub(case, torch.device(DEV)))


@pytest.mark.parametrize("c", H.LAYOUTS, ids=H.case_id)
def test_group_layouts(c):
    """b. Four groups, each with its own FCBlock: an empty group in the middle, empty leading groups, boundaries that are no multiple
    of 32.  One further hub block takes no part: its gradient must be exactly zero.  And the groups do not see each other: group g's
    rows of msg, x.grad and h.grad are bit for bit those of a launch with that group alone (so are its weight gradients: the same
    chunks in the same order)."""
    dev = torch.device(DEV)
    case, _, _ = H.reference(*c, H.seed_of(*c))
    got = H.run_hub(case, dev, extra_block=(1, 2) if c[:2] == (3, 3) else (3, 3))
    _check(c, got)
    assert float(got["extra"][0].abs().max()) == 0.0 and float(got["extra"][1].abs().max()) == 0.0
    lo = 0
    for g, n in enumerate(c[2]):
        if n:
            alone = H.run_hub(H.slice_case(case, g), dev)
            for k in ("msg", "gx", "gh"):
                assert torch.equal(got[k][lo:lo + n], alone[k]), (g, k)
            assert torch.equal(got["dW2"][g], alone["dW2"][0]) and torch.equal(got["db2"][g], alone["db2"][0]), g
        lo += n


@pytest.mark.parametrize("c", H.CHUNKED, ids=H.case_id)
def test_weight_gradient_chunking(c):
    """c. Sizes at which tp_train_dw_kernel's scale-dependent parts act (chunks = max(1, min(96, blocks // 4)), bpc = ceil(blocks /
    chunks)).  E = 1153: 37 blocks in 9 chunks of 5 -- chunk 7 holds two blocks, chunk 8 none (n_blk = -3) and must write an exactly
    zero partial block; grid.y = 16, the first launch in which the XCD remap is not the identity; grid.x = 10 / 12 / 13 / 14 with dead
    tile slots in the last workgroup at (0,1) and (3,3).  E = 2145: 68 blocks in 17 chunks of 4, grid.y padded to 24 (rows 17..23 exit),
    the last block holds one edge; at every level pair, because at E = 1153 the one remapped row is the empty chunk, so that only here
    LIVE chunks sit in rows >= 8.  [1153, 300, 33]: chunks [9, 2, 1], the later groups start at chunk 9 and 11 and at edges 1153 and
    1453.  The bound's fp32 sum length is 32 * bpc from that rule (160, 128, [160, 160, 64] edges), not read back from the library."""
    case, _, _ = H.reference(*c, H.seed_of(*c))
    got = H.run_hub(case, torch.device(DEV))
    _check(c, got)
    part = got["partial"]
    assert part.shape[0] == sum(H.dw_chunks(n)[0] for n in c[2]) and bool(torch.isfinite(part).all())
    # a chunk that owns at least one block writes a nonzero partial block, a chunk past the group's last block an exactly zero one
    # (chunk 8 of the 1153-edge group); every block was NaN before the launch
    row = 0
    for n in c[2]:
        k, bpc = H.dw_chunks(n)
        used = -(-(-(-n // 32)) // bpc)
        assert (n != 1153 or (k, used) == (9, 8)) and (n != 2145 or (k, used) == (17, 17))
        for j in range(k):
            assert (float(part[row + j].abs().max()) > 0.0) == (j < used), (n, j)
        row += k
    assert row == part.shape[0] and part.shape[1] == H.dims(c[0], c[1])["wp"] * 97


def test_weight_gradient_chunk_cap(monkeypatch):
    """c. The cap binds: DW_MAX_CHUNKS = 3 at E = 600 gives 19 blocks in 3 chunks of 7, the last one with 5 -- a chunk of 224 edges
    summed in fp32 (n = 224 + 11)."""
    from confidence_bootstrapping_amd import train_ops
    monkeypatch.setattr(train_ops, "DW_MAX_CHUNKS", 3)
    c = H.CAPPED
    case, _, _ = H.reference(*c, H.seed_of(*c))
    got = H.run_hub(case, torch.device(DEV))
    assert got["partial"].shape[0] == 3 and all(float(got["partial"][j].abs().max()) > 0.0 for j in range(3))
    _check(c, got, cap=3)


@pytest.mark.parametrize("lv", [(3, 3), (0, 1)])
def test_dw_abi_at_caller_chosen_chunk_counts(lv):
    """d. cbd_tp_backward_dw_groups + cbd_partial_reduce through the C ABI.  E = 40 in 5 chunks: two blocks, bpc 1, so chunks 2..4 own
    no block and must write exactly zero partial blocks.  E = 2000 in ONE chunk (bpc 63: 2016 edges in one fp32 sum) and in the 15
    chunks of the Python rule (bpc 5; chunks 13 and 14 empty).  dW2p / db2p, mapped to the reference layout through the packer's map,
    against g_w64^T h64 and the column sums of g_w64; the two chunkings agree within the sum of their bounds."""
    dev = torch.device(DEV)
    worst = {}

    def compare(c, n_chunks):
        case, ref, ab = H.reference(*c, H.seed_of(*c))
        got = H.run_dw_abi(case, dev, [n_chunks])
        bpc = -(-(-(-c[2][0] // 32)) // n_chunks)
        bnd = H.bounds(case, ab, dw_edges=[32 * bpc])
        dW64, db64 = ref["gw"][0].t() @ case["h"].double(), ref["gw"][0].sum(0)
        r = {"dW2": H.ratio(got["dW2"][0], dW64, bnd["dW2"][0]), "db2": H.ratio(got["db2"][0], db64, bnd["db2"][0])}
        print(f"tp train dw ABI vs fp64, {H.case_id(c)} in {n_chunks} chunks of {bpc}: largest error / bound {H.fmt(r)}")
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        return got, bnd

    got, _ = compare((lv[0], lv[1], (40,)), 5)
    part = got["partial"]
    assert part.shape[0] == 5 and float(part[2:].abs().max()) == 0.0
    assert float(part[0].abs().max()) > 0.0 and float(part[1].abs().max()) > 0.0
    c = (lv[0], lv[1], (2000,))
    one, b1 = compare(c, 1)
    assert H.dw_chunks(2000) == (15, 5)
    many, b15 = compare(c, 15)
    assert float(many["partial"][13:].abs().max()) == 0.0 and float(many["partial"][12].abs().max()) > 0.0
    for k in ("dW2", "db2"):
        assert bool(((one[k][0] - many[k][0]).abs() <= b1[k][0] + b15[k][0]).all()), k
    assert all(v <= 1 for v in worst.values()), worst


@pytest.mark.parametrize("lv", [(0, 1), (3, 3)])
def test_gradient_padding_does_not_leak(lv):
    """e. Of g_msg only the columns below out_dim may be read: a full-width upstream gradient with nonzero values in columns
    out_dim..79 must give x.grad, h.grad, fc[3].weight.grad and fc[3].bias.grad bit for bit those of the zero-padded run."""
    dev = torch.device(DEV)
    c = (lv[0], lv[1], (65,))
    case, _, _ = H.reference(*c, H.seed_of(*c))
    d = H.dims(*lv)
    pad = torch.randn(65, H.NODE_STRIDE - d["out_dim"], generator=torch.Generator().manual_seed(77)) * 3.0 + 1.0
    clean, dirty = H.run_hub(case, dev), H.run_hub(case, dev, gout_pad=pad)
    for k in ("msg", "gx", "gh"):
        assert torch.equal(clean[k], dirty[k]), k
    assert torch.equal(clean["dW2"][0], dirty["dW2"][0]) and torch.equal(clean["db2"][0], dirty["db2"][0])
    _check(c, dirty, what="hub (dirty padding)")
