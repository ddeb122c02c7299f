"""The fine-tuning kernels besides the generic Linear and the tensor product -- the FCBlocks' first stage (csrc/train_fc.hip), the segmented
sums and their users (csrc/tp_train.hip, csrc/train_edge.hip), the irreps BatchNorm (csrc/train_norm.hip) and the two e3nn heads
(csrc/train_heads.hip) -- on their production entry points against float64 references on the CPU, within a-priori fp32 bounds per element.
The cases, the references, the counts n behind the bounds and the runners are in tests/train_kernel_helpers.py;
tests/test_train_kernel_bounds.py shows on the CPU that torch's own fp32 arithmetic meets the same bounds for every case here and that a
wrong term does not.  Every run is made twice and must repeat bit for bit.  Every test prints its largest error / bound ratios (pytest -s
shows them) before it asserts."""
import pytest
import torch

from tests import train_kernel_helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FC_SEED = 20240611


# ================================================================================================================ 1. first stage
def _fc_backward_check(case, got, p, what):
    """the gradients against fp64 autograd of F.linear(x, W, b) * M, M = [hid_gpu > 0] / (1 - p): the mask is the run's own"""
    M = (got["hid"] > 0).double().cpu() / (1.0 - p)
    ref, ab = H.fc_grads64(case, M)
    r = H.fc_grad_ratios(got, ref, H.fc_grad_bounds(case, ab))
    print(f"first stage vs fp64, {what}: largest error / bound {H.fmt(r)}")
    assert all(v <= 1 for v in r.values()), r


@pytest.mark.parametrize("sizes", H.FC_LAYOUTS, ids=H.fc_id)
def test_first_stage_without_dropout(sizes):
    """hid = relu(x W_g^T + b_g) within (96 + 2) u (|x||W|^T + |b|) outside the sign band (at most 0.1 % of the elements inside it, each
    matching one branch); gx, dW1, db1 within their bounds under the run's own mask.  [65537]: 1024 parts of 66 rows, part 992 holds 65,
    parts 993..1023 none (their partial blocks are exact zeros that the double sum adds)."""
    case = H.fc_case(sizes)
    pre, ab_pre = H.fc_pre64(sizes)
    got = H.run_fc(case, torch.device(DEV))
    worst, share = H.fc_check_forward(got["hid"], pre, H.FC_N_HID * H.U * ab_pre + H.FLOOR)
    print(f"first stage vs fp64, {H.fc_id(sizes)}, p = 0: hid error / bound {worst:.3f}, share inside the sign band {share:.2e}")
    assert worst <= 1
    _fc_backward_check(case, got, 0.0, f"{H.fc_id(sizes)}, p = 0")


@pytest.mark.parametrize("p", H.FC_DROPOUT[1:])
@pytest.mark.parametrize("sizes", H.FC_LAYOUTS, ids=H.fc_id)
def test_first_stage_with_dropout(sizes, p):
    """h1 is, element by element, 0 or bitwise h0 * fl32(1 / (1 - p)), and 0 where h0 is; the gradients are those of F.linear * M with the
    run's own mask M = [h1 > 0] / (1 - p); the same seed and call give the same mask, another call another one"""
    dev = torch.device(DEV)
    case = H.fc_case(sizes)
    h0 = H.run_fc(case, dev)["hid"]
    got = H.run_fc(case, dev, p=p, seed=FC_SEED, call=1)                   # run twice inside: the same seed and call, the same mask
    h1 = got["hid"]
    scaled = h0 * torch.tensor(H.fc_scale32(p), dtype=torch.float32, device=dev)
    kept = h1 != 0
    assert torch.equal(h1[kept], scaled[kept]) and float(h1[h0 == 0].abs().sum()) == 0.0
    assert bool(((h1 == 0) | (h1 == scaled)).all())
    other = H.run_fc(case, dev, p=p, seed=FC_SEED, call=2)["hid"]
    act = h0 > 0
    if int(act.sum()) >= 40:                                              # 96 elements and more: two independent masks differ
        assert not torch.equal(other != 0, kept)
    if int(act.sum()) >= 20000:
        share = float((kept & act).sum() / act.sum())
        assert abs(share - (1 - p)) < 0.01, share
    _fc_backward_check(case, got, p, f"{H.fc_id(sizes)}, p = {p}")


@pytest.mark.parametrize("sizes", [s for s in H.FC_LAYOUTS if len(s) > 1], ids=H.fc_id)
def test_first_stage_groups_do_not_see_each_other(sizes):
    """a group run alone gives bit for bit the outputs and gradients it gives among the others (without dropout: the mask's hash runs over
    the row index in the whole tensor)"""
    dev = torch.device(DEV)
    case = H.fc_case(sizes)
    got = H.run_fc(case, dev)
    lo = 0
    for k, n in enumerate(sizes):
        alone = H.run_fc(H.fc_slice(case, k), dev)
        assert torch.equal(got["hid"][lo:lo + n], alone["hid"]) and torch.equal(got["gx"][lo:lo + n], alone["gx"]), k
        assert torch.equal(got["dW"][k], alone["dW"][0]) and torch.equal(got["db"][k], alone["db"][0]), k
        lo += n


def test_first_stage_refuses_five_groups():
    sizes = (3, 4, 5, 6, 7)
    assert len(sizes) == H.FC_MAX_GROUPS + 1
    with pytest.raises(RuntimeError):
        H.run_fc(H.fc_case(sizes), torch.device(DEV))


# ================================================================================================================ 2. segmented sums
def _twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for t, u in zip(a, b):
        assert torch.equal(t, u)
    return a


@pytest.mark.parametrize("c", H.SEG_CASES, ids=lambda c: f"N{c[0]}-W{c[1]}")
def test_segment_sums(c):
    """scatter_sum (forward; its backward is a gather), gather_rows (backward) and -- for the even widths up to 80 -- gather_pad (backward,
    row stride 80 -> D) within (len + 2) u sum|v| per element; the gathers and the zero padding exact.  A NaN in the row of an edge that
    belongs to one node reaches that node's output only."""
    from confidence_bootstrapping_amd import train_ops
    dev = torch.device(DEV)
    N, W = c
    case = H.seg_case(N, W)
    counts, index = case["counts"], case["index"]
    idx = index.to(dev)
    train_ops.clear_csr_cache()
    r = {}

    def sums():
        v = case["vals"].to(dev).requires_grad_()
        out = train_ops.scatter_sum(v, idx, N)
        out.backward(case["g_rows"].to(dev))
        x = case["node"].to(dev).requires_grad_()
        y = train_ops.gather_rows(x, idx)
        y.backward(case["vals2"].to(dev))
        return out.detach(), v.grad, y.detach(), x.grad

    out, gv, y, gx = _twice(sums)
    ref, ab = H.seg_sum64(case["vals"], index, N)
    r["scatter_sum"] = H.ratio(out, ref, H.seg_bounds(counts, ab))
    assert torch.equal(gv.cpu(), case["g_rows"][index]) and torch.equal(y.cpu(), case["node"][index])
    ref2, ab2 = H.seg_sum64(case["vals2"], index, N)
    r["gather_rows bwd"] = H.ratio(gx, ref2, H.seg_bounds(counts, ab2))
    if W % 2 == 0 and W <= 80:
        def pad():
            x = case["node"].to(dev).requires_grad_()
            rows = train_ops.gather_pad(x, idx)
            rows.backward(case["g80"].to(dev))
            return rows.detach(), x.grad
        rows, gxp = _twice(pad)
        assert rows.shape == (index.numel(), 80) and torch.equal(rows.cpu(), torch.nn.functional.pad(case["node"], (0, 80 - W))[index])
        ref3, ab3 = H.seg_sum64(case["g80"][:, :W], index, N)
        r["gather_pad bwd"] = H.ratio(gxp, ref3, H.seg_bounds(counts, ab3))
    print(f"segmented sums vs fp64, N = {N} ({H.seg_kernel(N)}), W = {W}: largest error / bound {H.fmt(r)}")
    assert all(v <= 1 for v in r.values()), r
    if N > 1:
        row = int(torch.nonzero(counts == 17)[0])
        e = int(torch.nonzero(index == row)[0])
        v = case["vals"].clone()
        v[e] = float("nan")
        bad = train_ops.scatter_sum(v.to(dev), idx, N)
        others = torch.arange(N, device=dev) != row
        assert bool(torch.isnan(bad[row]).all()) and torch.equal(bad[others], out[others])


@pytest.mark.parametrize("c", H.SEG_CASES, ids=lambda c: f"N{c[0]}-W{c[1]}")
def test_segment_mean(c):
    """scatter_mean forward within (len + 3) u sum|v| / count, its backward within 2 u |g| / count (count = 1 for a row without edges);
    width 3 takes the torch-op backward, the others cbd_segment_mean_backward"""
    from confidence_bootstrapping_amd import train_ops
    dev = torch.device(DEV)
    N, W = c
    case = H.seg_case(N, W)
    counts, index = case["counts"], case["index"]
    idx = index.to(dev)
    train_ops.clear_csr_cache()

    def mean():
        v = case["vals"].to(dev).requires_grad_()
        out = train_ops.scatter_mean(v, idx, N)
        out.backward(case["g_rows"].to(dev))
        return out.detach(), v.grad

    out, gv = _twice(mean)
    ref, ab = H.seg_sum64(case["vals"], index, N)
    cnt = counts.clamp(min=1).double()[:, None]
    gb64 = (case["g_rows"].double() / cnt)[index]
    r = {"scatter_mean": H.ratio(out, ref / cnt, H.seg_bounds(counts, ab, mean=True)),
         "scatter_mean bwd": H.ratio(gv, gb64, 2 * H.U * gb64.abs() + H.FLOOR)}
    print(f"segmented mean vs fp64, N = {N} ({H.seg_kernel(N)}), W = {W}: largest error / bound {H.fmt(r)}")
    assert all(v <= 1 for v in r.values()), r
    empty = counts == 0
    assert float(out[empty.to(dev)].abs().sum()) == 0.0


@pytest.mark.parametrize("c", H.EDGE_CAT_CASES, ids=lambda c: f"N{c[0]}-D{c[1]}")
def test_edge_cat_backward(c):
    """edge_cat: the forward is an exact copy; the node gradient's columns 0..31 within (len_src + len_dst + 1) u of the two magnitude
    sums, its columns >= 32 exactly zero; nodes that only send or only receive included"""
    from confidence_bootstrapping_amd import train_ops
    dev = torch.device(DEV)
    N, D = c
    case = H.edge_cat_case(N, D)
    src, dst = case["src"].to(dev), case["dst"].to(dev)
    train_ops.clear_csr_cache()

    def cat():
        ea, node = case["edge_attr"].to(dev).requires_grad_(), case["node"].to(dev).requires_grad_()
        out = train_ops.edge_cat(ea, node, src, dst)
        out.backward(case["g"].to(dev))
        return out.detach(), ea.grad, node.grad

    out, gea, gnode = _twice(cat)
    assert torch.equal(out.cpu(), torch.cat([case["edge_attr"], case["node"][:, :32][case["src"]], case["node"][:, :32][case["dst"]]], -1))
    assert torch.equal(gea.cpu(), case["g"][:, :32])
    ref, ab, bnd = H.edge_cat_ref64(case)
    r = H.ratio(gnode[:, :32], ref, bnd)
    print(f"edge_cat backward vs fp64, N = {N}, D = {D}: largest error / bound {r:.3f}")
    assert r <= 1 and gnode.shape == (N, D) and float(gnode[:, 32:].abs().sum()) == 0.0


# ================================================================================================================ 3. BatchNorm
BN_CASES = [(lay, N) for lay in H.BN_LAYOUTS for N in H.BN_NS]


def _bn_exact(case, got):
    D, res_dim = case["D"], case["res"].shape[1]
    assert got["y"].shape == (case["N"], D) and got["gx"].shape == (case["N"], case["ldx"])
    assert float(got["gx"][:, D:].abs().sum()) == 0.0                        # the padding columns of x carry no gradient
    assert torch.equal(got["gres"].cpu(), case["gout"][:, :res_dim])


@pytest.mark.parametrize("c", BN_CASES, ids=H.bn_id)
def test_batch_norm(c):
    """train-mode irreps BatchNorm + residual: y, gx, gw, gb and the running statistics against the fp64 restatement, in both data
    regimes (2 randn + 0.3; 0.5 randn + 30, where the fp32 rounding of the mean shows), at the 1024-thread stride boundaries"""
    (irreps, ldx, res_dim), N = c
    worst = {}
    for regime in H.BN_REGIMES:
        case, ref, ab, _ = H.bn_reference(irreps, ldx, res_dim, N, regime)
        got = H.run_bn(case, torch.device(DEV))
        _bn_exact(case, got)
        r = H.bn_ratios(got, ref, H.bn_bounds(ab))
        print(f"BatchNorm vs fp64, {irreps}, N = {N}, {regime}: largest error / bound {H.fmt(r)}")
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert all(v <= 1 for v in worst.values()), worst


@pytest.mark.parametrize("c", [(lay, N) for lay in H.BN_EXCL_LAYOUTS for N in H.BN_EXCL_NS], ids=H.bn_id)
def test_batch_norm_exclusion_ranges(c):
    """two ranges, a leading range, a range that ends at N: the live rows against the fp64 restatement over the live rows ALONE (not
    against the same kernel), the excluded rows exactly zero in y and gx whatever they hold (1e6)"""
    (irreps, ldx, res_dim), N = c
    dev = torch.device(DEV)
    worst = {}
    for regime in H.BN_REGIMES:
        case = H.bn_case(irreps, ldx, res_dim, N, regime)
        for ex in H.bn_excludes(N):
            live = H.bn_live(N, ex)
            ref, ab, _ = H.bn_ref64(case, live)
            got = H.run_bn(case, dev, exclude=ex, garbage=1e6)
            _bn_exact(case, got)
            dead = (~live).to(dev)
            assert float(got["y"][dead].abs().sum()) == 0.0 and float(got["gx"][dead].abs().sum()) == 0.0
            r = H.bn_ratios(got, ref, H.bn_bounds(ab), live=live)
            print(f"BatchNorm vs fp64 over the live rows, {irreps}, N = {N}, {regime}, exclude {ex}: largest error / bound {H.fmt(r)}")
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
    assert all(v <= 1 for v in worst.values()), worst


# ================================================================================================================ 4. heads
@pytest.mark.parametrize("c", H.CENTER_CASES, ids=H.head_id)
def test_centre_head(c):
    """CenterTpFn against train_forward.center_tensor_product in float64: out, gx, gw; the padding columns of gx exactly zero.  Rows 0, 1, 2
    (or the single row): a zero edge vector, one of norm 1e-20, one of norm 1e3.  n = 63 / 64 / 65: the 64-rows-per-block edge."""
    case, ref, ab = H.center_reference(c)
    got = H.run_head(case, torch.device(DEV), bond=False)
    r = H.head_ratios(got, ref, H.center_bounds(ab))
    print(f"centre head vs fp64, {H.head_id(c)}: largest error / bound {H.fmt(r)}")
    assert all(v <= 1 for v in r.values()), r
    assert float(got["gx"][:, H.HEAD_DIM:].abs().sum()) == 0.0


@pytest.mark.parametrize("c", H.BOND_CASES, ids=H.head_id)
def test_bond_head(c):
    """BondTpFn against train_forward.bond_tensor_product in float64; columns 0..31 and 68.. of gx exactly zero.  n = 1 / 3: the dead
    half-wave clamps to row n - 1 and takes part in the shuffles.  Row 3 (or the single row): edge parallel to bond."""
    case, ref, ab = H.bond_reference(c)
    got = H.run_head(case, torch.device(DEV), bond=True)
    r = H.head_ratios(got, ref, H.bond_bounds(ab))
    print(f"bond head vs fp64, {H.head_id(c)}: largest error / bound {H.fmt(r)}")
    assert all(v <= 1 for v in r.values()), r
    assert float(got["gx"][:, :32].abs().sum()) == 0.0 and float(got["gx"][:, 68:].abs().sum()) == 0.0
