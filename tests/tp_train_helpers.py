"""Shared by tests/test_tp_train_bounds.py (CPU) and tests/test_gpu_tp_train.py (GPU): an fp64 reference of one tensor-product layer
call of the fine-tuning step, its absolute companion, a-priori fp32 error bounds, seeded inputs and the runners of the production path
(train_ops.StreamHub + train_ops.TensorProductHubFn: cbd_tp_forward, cbd_tp_backward with gw = NULL, cbd_tp_backward_gh,
cbd_tp_backward_dw_groups, cbd_partial_reduce; csrc/tp_train.hip, csrc/train_fc.hip).

The layer call, per edge group g with its own second Linear (W2_g, b2_g):
    w = W2_g h + b2_g,   msg = FasterTensorProduct(x, [1, sqrt(3) vec], w),   loss = sum(msg * gout)
`tp_ref64` evaluates it with oracle.score_ref.faster_tensor_product in float64 and takes autograd gradients; `tp_abs64` restates the
same multilinear form with every input and every coefficient replaced by its magnitude, so that its value and its autograd gradients
are, per element, the sum of the absolute values of the terms of msg, gx, gh, dW2 and db2.

Bounds (the style of tests/test_gpu_linear.py): |got - ref64| <= n * u * abs_companion + FLOOR per element, u = 2^-24, FLOOR = 1e-30
(flushed denormals).  n is the length of the longest chain of fp32 roundings behind an element, counted from the kernels, never
fitted to an observed error:

  C_W = 4    the packed weight W2p = W2 * scale: scale = factor / sqrt(fan) is formed in fp32 by the packer (csrc/engine.hip
             conv_tile_rows: sqrtf(3) or sqrtf(1.5), sqrtf(fan), one division = 3 roundings) and the product is rounded once; the same
             four lie on the way back, fc[3].grad = dW2p * scale (StreamHub.pscale)
  C_MID = 3  the longest CG intermediate: a dot product of three (a cross product component has two roundings, scalar * v one)

  msg   KDIM + 1 + fan + C_W + C_MID + 1
        w: 96 fused multiply-adds on top of the bias (v_mfma_f32_32x32x2_f32: two products per step, counted as 96 + 1);
        the CG sum over the block's fan mids, one fma each; + 1 for `keep = v * sc + keep`, the scalar mids of a vector block folded
        in after the loop.  fan = 32 + n1o (0e), 32 + n1o + n1e (1o), n1o + n1e + n0o (1e), n1e + n0o (0o) of the INPUT level:
        the bound is taken per output column with its own block's fan
  gx    KDIM + 1 + NS + C_W + 3 + 3
        w as above; g_mid = sum over the block's output channels of w * g_msg: 16 fmas per lane half + the half sum for the 32
        channels of block 0e (17), 3 fmas + the half sum for a vector block (4): NS = 32 covers both; the transposed mid map (v . g:
        3, v x g: 2, g * v: 1) <= 3; and a column of the g_x tile receives `+=` from at most three output blocks.  The sum over the
        fan does not enter: every mid is its own term of g_x
  gh    wp + C_W + 6
        g_h = g_w W2p is ONE chain of MFMA k-steps over all wp packed rows (dead rows multiply zeros); g_w = mid (x) g_msg costs the
        mid (3) and a three-term dot product with g_msg (3).  wp = 32 * (fan0e + ceil(fan1o / 5) + ceil(fan1e / 5) + ceil(fan0o / 5)),
        blocks 1e / 0o only where the OUTPUT level has them: 1248, 1536, 1664, 1728 for (0,1), (1,2), (2,3), (3,3)
  dW2, db2    32 * g_bpc + 6 + 1 + C_W
        only the edges of one chunk are summed in fp32 (k-steps of tp_train_dw_kernel; db2p is the running sum of the A operand plus
        the half sum, at most as long); g_w as for gh (6); partial_reduce_kernel adds the chunks in double and rounds once (1); the
        scale on the way back (C_W).  g_bpc = ceil(ceil(E_g / 32) / chunks_g), chunks_g = max(1, min(cap, ceil(E_g / 32) // 4)), cap =
        train_ops.DW_MAX_CHUNKS (96): the documented rule, stated here and not read back from the library, so that the bound also
        pins that claim.  For torch's own fp32 autograd (the CPU check) the whole group is one fp32 sum: E_g + 6 + 1 + C_W.
"""
import ctypes as C
import functools
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
FLOOR = 1e-30
KDIM = 96
NS, NV = 32, 6
NODE_STRIDE = 80
LEVELS = [(0, 1), (1, 2), (2, 3), (3, 3)]
C_W, C_MID = 4, 3
DW_CAP = 96


def muls(level):
    """multiplicities (0e, 1o, 1e, 0o) of the node features at an irreps level"""
    return NS, NV if level >= 1 else 0, NV if level >= 2 else 0, NV if level >= 3 else 0


def dims(IN, OUT):
    i0e, i1o, i1e, i0o = muls(IN)
    o0e, o1o, o1e, o0o = muls(OUT)
    fans = (i0e + i1o, i0e + i1o + i1e, i1o + i1e + i0o, i1e + i0o)
    outs = (o0e, o1o, o1e, o0o)
    ntw = fans[0] + sum(-(-f // 5) for f, m in zip(fans[1:], outs[1:]) if m)
    return {"in_dim": i0e + 3 * i1o + 3 * i1e + i0o, "out_dim": o0e + 3 * o1o + 3 * o1e + o0o, "fans": fans, "outs": outs,
            "W": sum(f * m for f, m in zip(fans, outs)), "wp": 32 * ntw}


def dw_chunks(E, cap=DW_CAP):
    """(chunks, blocks per chunk) of a group of E edges: the rule of TensorProductHubFn.backward / cbd_tp_backward_dw_groups"""
    blocks = -(-E // 32)
    chunks = max(1, min(cap, blocks // 4))
    return chunks, -(-blocks // chunks)


# ---------------------------------------------------------------------------------------------------------------- inputs
def make_case(IN, OUT, groups, seed):
    """Seeded CPU inputs of one layer call: x = randn [E, in_dim], vec = normalised randn [E, 3], h = relu(randn) [E, 96] (exact zeros),
    gout = randn [E, out_dim], and per group W2 = randn / sqrt(96) [W, 96], b2 = randn [W]."""
    d = dims(IN, OUT)
    g = torch.Generator().manual_seed(seed)
    E = sum(groups)
    r = lambda *s: torch.randn(*s, generator=g)
    case = {"IN": IN, "OUT": OUT, "groups": tuple(int(n) for n in groups), "x": r(E, d["in_dim"]), "vec": F.normalize(r(E, 3), dim=-1),
            "h": torch.relu(r(E, KDIM)), "gout": r(E, d["out_dim"])}
    case["W2"] = [r(d["W"], KDIM) / math.sqrt(KDIM) for _ in groups]
    case["b2"] = [r(d["W"]) for _ in groups]
    return case


def slice_case(case, g):
    """group g of a case as a single-group case of its own"""
    lo = sum(case["groups"][:g])
    hi = lo + case["groups"][g]
    out = {k: case[k] for k in ("IN", "OUT")}
    out["groups"] = (case["groups"][g],)
    for k in ("x", "vec", "h", "gout"):
        out[k] = case[k][lo:hi]
    out["W2"], out["b2"] = [case["W2"][g]], [case["b2"][g]]
    return out


# the cases of tests/test_gpu_tp_train.py as (IN, OUT, groups); tests/test_tp_train_bounds.py runs every one of them on the CPU
RAGGED = [(i, o, (E,)) for i, o in LEVELS for E in (1, 31, 32, 33, 65)]
LAYOUTS = [(i, o, g) for i, o in ((3, 3), (1, 2)) for g in ((33, 0, 1, 64), (1, 1, 1, 1), (0, 0, 0, 5))]
# E = 1153: 37 blocks, 9 chunks of 5 (chunk 7 holds two blocks, chunk 8 none: n_blk = -3), the first launch with a remapped row >= 8;
# E = 2145: 68 blocks, 17 chunks of 4 (grid.y padded to 24), the last block holds one edge; [1153, 300, 33]: chunks [9, 2, 1], chunk
# offsets 9 and 11
# (at E = 1153 the only remapped row, 8, is the empty chunk: a wrong block count or row for by >= 8 shows from E = 2145 on, which is
# therefore run at every level pair -- each has its own grid.x in the remap)
CHUNKED = [(i, o, (1153,)) for i, o in LEVELS] + [(3, 3, (2145,)), (3, 3, (1153, 300, 33)), (0, 1, (1153, 300, 33))] + \
          [(i, o, (2145,)) for i, o in LEVELS[:3]]
CAPPED = (3, 3, (600,))        # with DW_MAX_CHUNKS = 3: 19 blocks, 3 chunks of 7, the last one holds 5
ABI = [(i, o, (E,)) for i, o in ((3, 3), (0, 1)) for E in (40, 2000)]
ALL_CASES = RAGGED + LAYOUTS + CHUNKED + [CAPPED] + ABI


def seed_of(IN, OUT, groups):
    return 100000 * IN + 10000 * OUT + 7 * sum(groups) + len(groups) + 13 * groups[0]


def case_id(c):
    return f"{c[0]}{c[1]}-" + "+".join(str(n) for n in c[2])


# ---------------------------------------------------------------------------------------------------------------- references
def _layer_grads(tp, case, dtype, absolute):
    """msg and the gradients of sum(msg * gout) through `tp(x, sh_vec, w, IN, OUT)` per group; every tensor in `dtype`."""
    IN, OUT, groups = case["IN"], case["OUT"], case["groups"]
    d = dims(IN, OUT)
    prep = (lambda t: t.detach().to(dtype).abs()) if absolute else (lambda t: t.detach().to(dtype))
    x, h = prep(case["x"]).requires_grad_(), prep(case["h"]).requires_grad_()
    vec, gout = prep(case["vec"]), prep(case["gout"])
    W2 = [prep(w).requires_grad_() for w in case["W2"]]
    b2 = [prep(b).requires_grad_() for b in case["b2"]]
    msgs, ws, lo = [], [], 0
    for g, n in enumerate(groups):
        if n == 0:
            ws.append(None)
            continue
        w = F.linear(h[lo:lo + n], W2[g], b2[g])
        ws.append(w)
        msgs.append(tp(x[lo:lo + n], vec[lo:lo + n], w, IN, OUT))
        lo += n
    msg = torch.cat(msgs) if msgs else x.new_zeros(0, d["out_dim"])
    live = [g for g, n in enumerate(groups) if n]
    leaves = [x, h] + [W2[g] for g in live] + [b2[g] for g in live] + [ws[g] for g in live]
    gs = torch.autograd.grad((msg * gout).sum(), leaves) if live else []
    k = len(live)
    out = {"msg": msg.detach(), "gx": gs[0] if live else torch.zeros_like(x), "gh": gs[1] if live else torch.zeros_like(h),
           "dW2": [torch.zeros_like(w) for w in W2], "db2": [torch.zeros_like(b) for b in b2], "gw": [None] * len(groups)}
    for j, g in enumerate(live):
        out["dW2"][g], out["db2"][g], out["gw"][g] = gs[2 + j], gs[2 + k + j], gs[2 + 2 * k + j]
    return out


def _oracle_tp(x, vec, w, IN, OUT):
    from oracle import score_ref as sr
    sh = torch.cat([torch.ones_like(vec[:, :1]), math.sqrt(3.0) * vec], 1)
    return sr.faster_tensor_product(x, sh, w, sr.IRREP_SEQ[IN], sr.IRREP_SEQ[OUT])


def _abs_cross(a, v):
    """magnitudes of the terms of a x v: component a_y b_z - a_z b_y becomes |a_y| |b_z| + |a_z| |b_y|; a [E, m, 3], v [E, 3]"""
    v = v[:, None, :]
    return torch.stack([a[..., 1] * v[..., 2] + a[..., 2] * v[..., 1],
                        a[..., 2] * v[..., 0] + a[..., 0] * v[..., 2],
                        a[..., 0] * v[..., 1] + a[..., 1] * v[..., 0]], dim=-1)


def _abs_tp(x, vec, w, IN, OUT):
    """The lmax = 1 tensor product with per-edge weights on MAGNITUDES: x, vec, w >= 0 elementwise; every coefficient positive."""
    E = x.shape[0]
    i0e, i1o, i1e, i0o = muls(IN)
    d = dims(IN, OUT)
    x0e = x[:, :i0e]
    x1o = x[:, i0e:i0e + 3 * i1o].reshape(E, i1o, 3)
    x1e = x[:, i0e + 3 * i1o:i0e + 3 * i1o + 3 * i1e].reshape(E, i1e, 3)
    x0o = x[:, i0e + 3 * i1o + 3 * i1e:]
    s3, r2 = math.sqrt(3.0), math.sqrt(2.0)
    v = s3 * vec                                                                  # |sh_1|; |sh_0| = 1
    mids = [torch.cat([x0e, (x1o * v[:, None, :]).sum(-1) / s3], dim=-1),
            torch.cat([x0e[:, :, None] * v[:, None, :], x1o, _abs_cross(x1e, v) / r2], dim=-2),
            torch.cat([_abs_cross(x1o, v) / r2, x1e, x0o[:, :, None] * v[:, None, :]], dim=-2),
            torch.cat([(x1e * v[:, None, :]).sum(-1) / s3, x0o], dim=-1)]
    out, start = [], 0
    for k, (fan, mo) in enumerate(zip(d["fans"], d["outs"])):
        if fan * mo == 0:
            continue
        wk = w[:, start:start + fan * mo].reshape(E, fan, mo) / math.sqrt(fan)
        start += fan * mo
        if k in (0, 3):
            out.append(torch.einsum("ef,efo->eo", mids[k], wk))
        else:
            out.append(torch.einsum("efc,efo->eoc", mids[k], wk).reshape(E, 3 * mo))
    return torch.cat(out, dim=-1)


def tp_ref64(case):
    """fp64 CPU form of one layer call: msg [E, out_dim], gx, gh, per group dW2 / db2 (zeros for an empty group) and gw = d loss / d w
    [E_g, W] (None for an empty group), by autograd through the oracle."""
    return _layer_grads(_oracle_tp, case, torch.float64, False)


def tp_abs64(case):
    """the absolute companion of tp_ref64: the same keys, every element the sum of the magnitudes of its terms"""
    return _layer_grads(_abs_tp, case, torch.float64, True)


def tp_torch32(case):
    """the oracle formula in float32 on the CPU with torch's own fp32 autograd"""
    return _layer_grads(_oracle_tp, case, torch.float32, False)


@functools.lru_cache(maxsize=None)
def reference(IN, OUT, groups, seed):
    """(case, tp_ref64, tp_abs64) of a seeded case, computed once per session and never modified"""
    case = make_case(IN, OUT, groups, seed)
    return case, tp_ref64(case), tp_abs64(case)


# ---------------------------------------------------------------------------------------------------------------- bounds
def bounds(case, ab, cap=DW_CAP, dw_edges=None):
    """elementwise bounds from the absolute companion `ab`; dW2 / db2 with n = 32 * g_bpc + 11 (dw_edges = None) or with the fp32 sum
    length per group given in dw_edges (a list: E_g for torch's autograd, 32 * bpc of a caller-chosen chunking)"""
    d = dims(case["IN"], case["OUT"])
    fan_col = torch.cat([torch.full((m * (1 if k in (0, 3) else 3),), float(f), dtype=torch.float64)
                         for k, (f, m) in enumerate(zip(d["fans"], d["outs"])) if m])
    assert fan_col.numel() == d["out_dim"]
    n_msg = KDIM + 1 + fan_col + C_W + C_MID + 1
    n_gx = KDIM + 1 + NS + C_W + 3 + 3
    n_gh = d["wp"] + C_W + 6
    out = {"msg": n_msg[None, :] * U * ab["msg"] + FLOOR, "gx": n_gx * U * ab["gx"] + FLOOR, "gh": n_gh * U * ab["gh"] + FLOOR,
           "dW2": [], "db2": []}
    for g, E in enumerate(case["groups"]):
        n_sum = 32 * dw_chunks(E, cap)[1] if dw_edges is None else dw_edges[g]
        n_dw = n_sum + 6 + 1 + C_W
        out["dW2"].append(n_dw * U * ab["dW2"][g] + FLOOR)
        out["db2"].append(n_dw * U * ab["db2"][g] + FLOOR)
    return out


def ratio(got, ref, bound):
    """largest |got - ref| / bound; 0 for an empty tensor"""
    if ref.numel() == 0:
        return 0.0
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / bound).max())


def ratios(got, ref, bnd):
    """worst error / bound ratio per tensor of one run (`got` as the runners return it: padded msg / gx are cut to their live columns)"""
    out_dim, in_dim = ref["msg"].shape[1], ref["gx"].shape[1]
    r = {"msg": ratio(got["msg"][:, :out_dim], ref["msg"], bnd["msg"]), "gx": ratio(got["gx"][:, :in_dim], ref["gx"], bnd["gx"]),
         "gh": ratio(got["gh"], ref["gh"], bnd["gh"])}
    r["dW2"] = max([ratio(a, b, c) for a, b, c in zip(got["dW2"], ref["dW2"], bnd["dW2"])] or [0.0])
    r["db2"] = max([ratio(a, b, c) for a, b, c in zip(got["db2"], ref["db2"], bnd["db2"])] or [0.0])
    return r


def fmt(r):
    return ", ".join(f"{k}={v:.3f}" for k, v in r.items())


# ---------------------------------------------------------------------------------------------------------------- GPU runners
def _fcblock(W2, b2, dev):
    from confidence_bootstrapping_amd.score_model import FCBlock
    fc = FCBlock(KDIM, KDIM, W2.shape[0], 0.0)
    with torch.no_grad():
        fc[3].weight.copy_(W2)
        fc[3].bias.copy_(b2)
    return fc.to(dev)


def run_hub(case, dev, gout_pad=None, extra_block=None):
    """The production path on the device: a StreamHub over the case's FCBlocks (one per group, plus -- extra_block = (IN, OUT) -- one that
    takes no part), hub.pack(), TensorProductHubFn.apply, backward under gout.  gout_pad [E, 80 - out_dim]: what the padding columns
    of the upstream gradient hold (default zeros).  The whole step runs twice and the two runs must agree bit for bit.
    Returns msg [E, 80], gx [E, 80], gh [E, 96], dW2 / db2 per group (fc[3].weight.grad / fc[3].bias.grad), `extra` (the two
    gradients of the idle block, or None) and `partial` (the per-chunk blocks of the weight-gradient pass, see below)."""
    from confidence_bootstrapping_amd.train_ops import StreamHub, TensorProductHubFn
    IN, OUT, groups = case["IN"], case["OUT"], case["groups"]
    d = dims(IN, OUT)
    fcs = [_fcblock(w, b, dev) for w, b in zip(case["W2"], case["b2"])]
    blocks = [(fc, IN, OUT) for fc in fcs]
    idle = None
    if extra_block is not None:
        wi = dims(*extra_block)["W"]
        idle = _fcblock(torch.ones(wi, KDIM), torch.ones(wi), dev)
        blocks.insert(1, (idle, extra_block[0], extra_block[1]))          # in the middle of the hub's buffers, not at their end
    hub = StreamHub(blocks, dev)
    ids = [hub.block(fc) for fc in fcs]
    x80 = F.pad(case["x"], (0, NODE_STRIDE - d["in_dim"])).to(dev)
    vec4 = F.pad(case["vec"], (0, 1)).to(dev)
    hd = case["h"].to(dev)
    g80 = F.pad(case["gout"], (0, NODE_STRIDE - d["out_dim"]))
    if gout_pad is not None:
        g80[:, d["out_dim"]:] = gout_pad
    g80 = g80.to(dev)

    # the partial blocks of the weight-gradient pass live in train_ops' persistent scratch buffer: NaN-filled before every run, so that
    # a block the kernel leaves unwritten shows in the reduced gradient, and returned as `partial` [chunks of all groups, wp * 97]
    from confidence_bootstrapping_amd import train_ops
    width = d["wp"] * KDIM + d["wp"]
    n_part = sum(dw_chunks(n, train_ops.DW_MAX_CHUNKS)[0] for n in groups if n)

    def once():
        for fc, _, _ in blocks:
            fc.zero_grad(set_to_none=True)
        train_ops._dw_scratch(n_part * width, dev).fill_(float("nan"))
        hub.pack()
        x, h = x80.clone().requires_grad_(), hd.clone().requires_grad_()
        msg = TensorProductHubFn.apply(x, vec4, h, hub.big, hub, IN, OUT, tuple(groups), tuple(ids))
        msg.backward(g80)
        torch.cuda.synchronize()
        out = {"msg": msg.detach().clone(), "gx": x.grad.clone(), "gh": h.grad.clone(),
               "dW2": [fc[3].weight.grad.clone() for fc in fcs], "db2": [fc[3].bias.grad.clone() for fc in fcs],
               "extra": None if idle is None else (idle[3].weight.grad.clone(), idle[3].bias.grad.clone()),
               "partial": train_ops._dw_scratch(n_part * width, dev).view(n_part, width).clone()}
        assert fcs[0][0].weight.grad is None or float(fcs[0][0].weight.grad.abs().max()) == 0.0
        return out

    a, b = once(), once()
    for k in ("msg", "gx", "gh"):
        assert torch.equal(a[k], b[k]), k
    for k in ("dW2", "db2"):
        for t, u in zip(a[k], b[k]):
            assert torch.equal(t, u), k
    return a


def run_dw_abi(case, dev, n_chunks):
    """cbd_tp_backward_dw_groups + cbd_partial_reduce through the C ABI at caller-chosen chunk counts (one per non-empty group; the case
    must have no empty group).  Every buffer starts NaN-filled.  Returns the partial blocks [sum(n_chunks), wp * 96 + wp] and, per
    group, dW2 [W, 96] / db2 [W] in the reference layout as float64 (dW2p / db2p mapped back through the packer's map and scale, as
    StreamHub does for fc[3].grad)."""
    from confidence_bootstrapping_amd.engine import load_library, _check
    from confidence_bootstrapping_amd.train_ops import StreamHub, _stream_handle
    lib = load_library()
    IN, OUT, groups = case["IN"], case["OUT"], case["groups"]
    d = dims(IN, OUT)
    wp, W = d["wp"], d["W"]
    assert all(n > 0 for n in groups) and len(n_chunks) == len(groups)
    hub = StreamHub([(_fcblock(case["W2"][0], case["b2"][0], dev), IN, OUT)], dev)       # for its parameter -> gradient-slot map only
    assert hub.n_grad == wp * KDIM + wp and hub.p2g.numel() == W * KDIM + W
    P = lambda t: C.c_void_p(t.data_ptr())
    x80 = F.pad(case["x"], (0, NODE_STRIDE - d["in_dim"])).to(dev)
    vec4 = F.pad(case["vec"], (0, 1)).to(dev)
    hd = case["h"].to(dev)
    g80 = F.pad(case["gout"], (0, NODE_STRIDE - d["out_dim"])).to(dev)
    ng, width = len(groups), wp * KDIM + wp
    part = torch.full((sum(n_chunks), width), float("nan"), device=dev, dtype=torch.float32)
    ge = (C.c_int64 * ng)(*groups)
    nc = (C.c_int32 * ng)(*n_chunks)
    _check(lib.cbd_tp_backward_dw_groups(IN, OUT, ng, ge, nc, P(x80), P(vec4), P(hd), P(g80), P(part), _stream_handle()))
    outs = [torch.full((width,), float("nan"), device=dev, dtype=torch.float32) for _ in groups]
    oa = (C.c_void_p * ng)(*[o.data_ptr() for o in outs])
    ob = (C.c_void_p * ng)(*[o.data_ptr() + 4 * wp * KDIM for o in outs])
    _check(lib.cbd_partial_reduce(ng, nc, width, wp * KDIM, P(part), oa, ob, _stream_handle()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(part).all())
    res = {"partial": part, "dW2": [], "db2": []}
    for o in outs:
        flat = (o.double().index_select(0, hub.p2g) * hub.pscale.double()).cpu()
        res["dW2"].append(flat[:W * KDIM].view(W, KDIM))
        res["db2"].append(flat[W * KDIM:])
    return res
