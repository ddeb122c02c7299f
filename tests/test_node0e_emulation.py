"""CPU emulation of the node-major 0e path of the fp32 74 -> 74 layers (csrc/tp_node0e.hip) on the REAL packed weight stream, compared
with the oracle's FCBlock + FasterTensorProduct summed over each aggregating node's edges.

Order of operations emulated: h_e from the stream's three first-Linear tiles (32 edges of one node per wave pass), the per-node
aggregates A[k][j] = sum_e h_e[k] T_e[j] kept in the second Linear's B-operand order (slot s of lane half hf), S[j] = sum_e T_e[j], then
D[w][node] = sum_j (0e tile j) x A[:, j, node] with the nodes on the MFMA N dimension, plus sum_j b2_j[w] S[j].
"""
import numpy as np
import torch

from oracle import score_ref as sr
from oracle.e3nn_ref import sh_l1
from tests.test_pack_emulation import KSTEPS, TILE_W, COL_1O, gemm_tile, row_of

NS, NMID = 32, 38
N0E_S_OFF = NMID * 96             # common.h
N0E_ROW = N0E_S_OFF + 64


def mids(xrow, v):
    """T_e[j]: the 38 mids of block 0e (x0e_dst[u], x1o_dst[u] . v)"""
    t = np.zeros((xrow.shape[0], NMID))
    t[:, :NS] = xrow[:, :NS]
    for u in range(6):
        t[:, NS + u] = np.einsum("ec,ec->e", xrow[:, COL_1O + 3 * u:COL_1O + 3 * u + 3], v)
    return t


def emulate_node0e(stream, xin, xrow, v, deg):
    """The two kernels of tp_node0e.hip lane by lane: the build kernel's LDS tiles hT[edge][k] / tT[edge][mid], its six 32x32 MFMA
    accumulators D[b][jb] (k block b, mid block jb, edges on K), their store into the node's abuf row (lane (col, hf), register r ->
    row[col * 96 + 48 hf + 16 b + r], S at N0E_S_OFF), and the gemm kernel's B operand read back from that row."""
    nt = 3 + 38 + 9 + 4 + 3 - 1                                   # conv_shape(3, 3, merged=True).ntiles
    wts, bias = stream[:nt * TILE_W].reshape(nt, TILE_W), stream[(nt + 1) * TILE_W:].reshape(nt, 32)
    lanes = np.arange(64)
    j, hf = lanes & 31, lanes >> 5
    n_nodes = len(deg)
    abuf = np.full((n_nodes, N0E_ROW), np.nan)                    # every slot the gemm kernel reads must be written
    T = mids(xrow, v)
    e0 = 0
    for n, d in enumerate(deg):
        D = np.zeros((3, 2, 32, 32))                              # [k block][mid block][row][col]
        S = np.zeros(64)
        for c0 in range(0, d, 32):                                 # 32 edges of the node per pass
            nc = min(32, d - c0)
            ec = e0 + c0 + np.minimum(j, nc - 1)                   # lanes past the node's edges read its last edge, mids zeroed
            Bx = np.zeros((KSTEPS, 64))
            for s in range(KSTEPS):
                Bx[s] = xin[ec, 32 * (s // 16) + 16 * hf + (s % 16)]
            h1 = np.zeros((KSTEPS, 64))
            for m in range(3):
                h1[16 * m:16 * m + 16] = np.maximum(gemm_tile((wts[m], bias[m]), Bx), 0)
            hT = np.zeros((32, 96))
            tT = np.zeros((32, 64))
            for lane in range(64):
                for m in range(3):
                    for r in range(16):
                        hT[lane & 31, 32 * m + row_of(r, lane >> 5)] = h1[16 * m + r, lane]
            for e in range(nc):
                tT[e, :NMID] = T[ec[e]]
            S[:NMID] += tT[:nc, :NMID].sum(0)
            for s in range((nc + 1) // 2):                         # MFMA k-step s: lane half hf supplies edge 2s + hf
                for b in range(3):
                    for jb in range(2):
                        for kk in range(2):
                            D[b, jb] += np.outer(hT[2 * s + kk, 32 * b:32 * b + 32], tT[2 * s + kk, 32 * jb:32 * jb + 32])
        for lane in range(64):                                     # stores of the build kernel
            c, h = lane & 31, lane >> 5
            for b in range(3):
                for r in range(16):
                    abuf[n, c * 96 + 48 * h + 16 * b + r] = D[b, 0, row_of(r, h), c]
                    if c < NMID - NS:
                        abuf[n, (NS + c) * 96 + 48 * h + 16 * b + r] = D[b, 1, row_of(r, h), c]
            if lane < NMID:
                abuf[n, N0E_S_OFF + lane] = S[lane]
        e0 += d
    # gemm kernel: lane (node = lane & 31, hf) reads B.v[i] = row[jj * 96 + 48 hf + i] for 0e tile jj
    out = np.zeros((n_nodes, NS))
    acc = np.zeros((16, 64))
    for jj in range(NMID):
        B = np.zeros((KSTEPS, 64))
        for lane in range(64):
            if (lane & 31) < n_nodes:
                B[:, lane] = abuf[lane & 31, jj * 96 + 48 * (lane >> 5):jj * 96 + 48 * (lane >> 5) + 48]
        acc += gemm_tile((wts[3 + jj], np.zeros(32)), B)
    for lane in range(64):
        node, h = lane & 31, lane >> 5
        if node >= n_nodes:
            continue
        for reg in range(16):
            w = row_of(reg, h)
            out[node, w] = acc[reg, lane] + sum(bias[3 + jj][w] * abuf[node, N0E_S_OFF + jj] for jj in range(NMID))
    assert not np.isnan(out).any()
    return out


def test_node_major_0e_reproduces_per_node_message_sums():
    from confidence_bootstrapping_amd.engine import pack_conv_stream
    g = torch.Generator().manual_seed(33)
    in_irr, out_irr = sr.IRREP_SEQ[3], sr.IRREP_SEQ[3]
    W = sr.faster_tp_weight_numel(in_irr, out_irr)
    w1, b1 = torch.randn(96, 96, generator=g) / 8, torch.randn(96, generator=g) / 4
    w2, b2 = torch.randn(W, 96, generator=g) / 8, torch.randn(W, generator=g) / 4
    stream = pack_conv_stream(3, 3, w1.numpy(), b1.numpy(), w2.numpy(), b2.numpy(), merged=True).astype(np.float64)
    deg = [1, 0, 7, 33, 24, 70]                                    # C2-like degrees: receptor nodes ~16-24, ligand nodes with many cross edges
    E = sum(deg)
    in_dim = sr.e3.Irreps(in_irr).dim
    xin = torch.randn(E, 96, generator=g)
    xd = torch.randn(E, in_dim, generator=g)
    vec = torch.randn(E, 3, generator=g)
    hid = torch.relu(xin.double() @ w1.double().T + b1.double())
    tpw = hid @ w2.double().T + b2.double()
    msg = sr.faster_tensor_product(xd.double(), sh_l1(vec.double()), tpw, in_irr, out_irr).numpy()
    ref = np.zeros((len(deg), NS))
    e0 = 0
    for n, d in enumerate(deg):
        ref[n] = msg[e0:e0 + d, :NS].sum(0)
        e0 += d
    xrow = np.zeros((E, 80))
    xrow[:, :in_dim] = xd.double().numpy()
    v = torch.nn.functional.normalize(vec.double(), dim=-1).numpy()
    got = emulate_node0e(stream, xin.double().numpy(), xrow, v, deg)
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5 * np.abs(ref).max())
    assert np.all(got[1] == 0)
