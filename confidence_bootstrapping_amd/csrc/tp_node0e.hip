// Block 0e of the 74 -> 74 exact-fp32 layers, aggregated BEFORE the second Linear.
//
// The message of an edge is linear in its per-edge weights w_e = W2 h_e + b2, and messages are summed per aggregating node before
// anything nonlinear happens, so for the 0e output block (mid index j, 38 mids: x0e_dst[u], x1o_dst[u] . v)
//   out0e_n[w] = sum_{e in n} sum_j T_e[j] (W2_j h_e + b2_j)[w]
//              = sum_j sum_k W2_j[w][k] A_n[k][j]  +  sum_j b2_j[w] S_n[j],     A_n[k][j] = sum_{e in n} h_e[k] T_e[j],  S_n[j] = sum_{e in n} T_e[j]
// Two kernels per launch of the edge kernel (which then runs the vector blocks only, ConvGroup::i0e_lo = i0e_hi = t0e):
//   node0e_build_kernel  one wave per NPW aggregating nodes: h_e (first Linear, as in tp_conv_kernel) for 32 edges of the node at a time,
//                        A_n += H^T T on the matrix cores (K = edges), S_n on the VALU; A_n / S_n -> abuf
//   node0e_gemm_kernel   one wave per 32 aggregating nodes: D[w][node] = sum_j W2_j A[:, j, node] with the group's existing 0e weight
//                        tiles as the A operand (unchanged stream), nodes on the MFMA N dimension; + the bias term; -> out0e[node][32]
// Each node's sums run over its own CSR edge range in a fixed order: results do not depend on the tiling or on the co-scheduled batches.
#include "kernels.h"
#include "tp_conv_dev.h"

namespace cbd {

constexpr int N0E_MIDS = NS + NV;                     // 38 mids of the 0e block (74 -> 74 layers)
constexpr int N0E_NPW = 4;                            // aggregating nodes per wave of the build kernel
static_assert(N0E_S_OFF == N0E_MIDS * KDIM, "abuf row layout");

// abuf row of a node: [j][hf][48] = A[k(s, hf)][j] in the B-operand order of the second Linear (k(s, hf) = 32(s/16) + (s&3) + 8((s&15)>>2)
// + 4hf, the C/D layout of the first Linear), then S[38]
__global__ __launch_bounds__(64) void node0e_build_kernel(N0eArgs args) {
  // row strides padded by one float: lane = edge writes a column of the tile, and a power-of-two-multiple stride put those 32 stores
  // on one or two LDS banks (PMC: bank conflicts were 77 % of the kernel's LDS cycles with strides 96 / 64)
  constexpr int HS = KDIM + 1, TS = 64 + 1;
  __shared__ float hT[WAVE_EDGES * HS];    // [edge][k]
  __shared__ float tT[WAVE_EDGES * TS];    // [edge][j], j >= 38 zero
  const int lane = threadIdx.x, j = lane & 31, hf = lane >> 5;
  int t = blockIdx.x, g = 0;
  for (; g < args.n_groups; ++g) {
    const int nw = (args.g[g].n_nodes + N0E_NPW - 1) / N0E_NPW;
    if (t < nw) break;
    t -= nw;
  }
  if (g >= args.n_groups) return;
  const N0eGroup& G = args.g[g];
  const GPtr<f32x4> gu = (GPtr<f32x4>)reinterpret_cast<const f32x4*>(G.wstream);
  f32x4 a[OpsF32::NFRAG];
  OpsF32::load_first(a, gu, lane);                    // the three first-Linear tiles stay in registers for all nodes of the wave
  const f32x4* const gb = reinterpret_cast<const f32x4*>(G.wstream + (size_t)(conv_shape(3, 3, true).ntiles + 1) * TILE_W_FLOATS);
  for (int i = lane; i < WAVE_EDGES * TS; i += 64) tT[i] = 0.f;

  for (int q = 0; q < N0E_NPW; ++q) {
    const int k = t * N0E_NPW + q;
    if (k >= G.n_nodes) break;
    const int s0 = G.start[k], n = G.cnt[k];
    f32x16 D[3][2];
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) { D[b][0][r] = 0.f; D[b][1][r] = 0.f; }
    float S = 0.f;
    for (int c0 = 0; c0 < n; c0 += WAVE_EDGES) {
      const int nc = n - c0 < WAVE_EDGES ? n - c0 : WAVE_EDGES;
      const bool valid = j < nc;
      const int ec = s0 + c0 + (valid ? j : nc - 1);
      const int src_r = G.src[ec], dst = G.dst[ec], aidx = G.attr_idx[ec];
      const f32x4 vv = reinterpret_cast<const f32x4*>(G.vec)[ec];
      OpsF32::Act Bx;
      const f32x4* pa = reinterpret_cast<const f32x4*>(G.attr + (size_t)aidx * 32 + 16 * hf);
#pragma unroll
      for (int u = 0; u < 4; ++u) OpsF32::set_in(Bx, 0, u, pa[u]);
      // first Linear exactly as tp_conv_kernel: b1 + W1s x_src + W1d x_dst (per-node projections), then the K = 32 edge-attribute part
      const f32x4* const p_s = reinterpret_cast<const f32x4*>(G.psrc + (size_t)src_r * KDIM + 4 * hf);
      const f32x4* const p_d = reinterpret_cast<const f32x4*>(G.pdst + (size_t)dst * KDIM + 4 * hf);
      OpsF32::Act h;
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        f32x16 acc;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const f32x4 b = gb[8 * m + 2 * u + hf], x = p_s[8 * m + 2 * u], y = p_d[8 * m + 2 * u];
          acc[4 * u + 0] = b.x + x.x + y.x; acc[4 * u + 1] = b.y + x.y + y.y;
          acc[4 * u + 2] = b.z + x.z + y.z; acc[4 * u + 3] = b.w + x.w + y.w;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const f32x4 w = a[4 * m + s];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, Bx.v[4 * s + 0], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, Bx.v[4 * s + 1], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, Bx.v[4 * s + 2], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, Bx.v[4 * s + 3], acc, 0, 0, 0);
        }
        OpsF32::set_hidden(h, m, acc);
      }
      // the mids of the edge (zero for lanes past the node's edges)
      const float* xr = G.node_in + (size_t)dst * NODE_STRIDE;
      float tv[16], dv[3];
      {
        const f32x4* px = reinterpret_cast<const f32x4*>(xr + 16 * hf);
#pragma unroll
        for (int u = 0; u < 4; ++u) { const f32x4 x = px[u]; tv[4 * u] = x.x; tv[4 * u + 1] = x.y; tv[4 * u + 2] = x.z; tv[4 * u + 3] = x.w; }
#pragma unroll
        for (int o = 0; o < 3; ++o) {
          const float* p = xr + COL_1O + 3 * (3 * hf + o);
          dv[o] = p[0] * vv.x + p[1] * vv.y + p[2] * vv.z;
        }
      }
      __syncthreads();   // the previous chunk's reads of hT / tT are complete
#pragma unroll
      for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) hT[j * HS + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * hf] = h.v[16 * m + r];
#pragma unroll
      for (int u = 0; u < 16; ++u) tT[j * TS + 16 * hf + u] = valid ? tv[u] : 0.f;
#pragma unroll
      for (int o = 0; o < 3; ++o) tT[j * TS + NS + 3 * hf + o] = valid ? dv[o] : 0.f;
      __syncthreads();
      if (lane < N0E_MIDS)
        for (int e = 0; e < nc; ++e) S += tT[e * TS + lane];
      // A += H^T T: D[k row][j col], K = edge pairs (lane half hf supplies edge 2s + hf; an odd count's last pair has a zero mid row)
      const int np = (nc + 1) >> 1;
      for (int s = 0; s < np; ++s) {
        const int e = 2 * s + hf;
        const float h0 = hT[e * HS + j], h1 = hT[e * HS + 32 + j], h2 = hT[e * HS + 64 + j];
        const float t0 = tT[e * TS + j], t1 = tT[e * TS + 32 + j];
        D[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(h0, t0, D[0][0], 0, 0, 0);
        D[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(h1, t0, D[1][0], 0, 0, 0);
        D[2][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(h2, t0, D[2][0], 0, 0, 0);
        D[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(h0, t1, D[0][1], 0, 0, 0);
        D[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(h1, t1, D[1][1], 0, 0, 0);
        D[2][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(h2, t1, D[2][1], 0, 0, 0);
      }
    }
    // lane (col j, hf) holds A[k = 32b + (r&3) + 8(r>>2) + 4hf][mid j] in D[b][.][r]: exactly B-operand slot 16b + r of lane half hf
    float* row = G.abuf + (size_t)k * N0E_ROW;
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        reinterpret_cast<f32x4*>(row + j * KDIM + 48 * hf + 16 * b)[r4] =
            f32x4{D[b][0][4 * r4], D[b][0][4 * r4 + 1], D[b][0][4 * r4 + 2], D[b][0][4 * r4 + 3]};
        if (j < NV)
          reinterpret_cast<f32x4*>(row + (NS + j) * KDIM + 48 * hf + 16 * b)[r4] =
              f32x4{D[b][1][4 * r4], D[b][1][4 * r4 + 1], D[b][1][4 * r4 + 2], D[b][1][4 * r4 + 3]};
      }
    if (lane < N0E_MIDS) row[N0E_S_OFF + lane] = S;
  }
}

__global__ __launch_bounds__(64) void node0e_gemm_kernel(N0eArgs args) {
  const int lane = threadIdx.x, j = lane & 31, hf = lane >> 5;
  int t = blockIdx.x, g = 0;
  for (; g < args.n_groups; ++g) {
    const int nw = (args.g[g].n_nodes + WAVE_EDGES - 1) / WAVE_EDGES;
    if (t < nw) break;
    t -= nw;
  }
  if (g >= args.n_groups) return;
  const N0eGroup& G = args.g[g];
  const int k = t * WAVE_EDGES + j;
  const int kc = k < G.n_nodes ? k : G.n_nodes - 1;
  constexpr int T0 = 3;                                // first 0e tile of the stream
  const GPtr<f32x4> gu = (GPtr<f32x4>)reinterpret_cast<const f32x4*>(G.wstream);
  const float* bias = G.wstream + (size_t)(conv_shape(3, 3, true).ntiles + 1) * TILE_W_FLOATS;
  f32x4 a[OpsF32::NFRAG];
#pragma unroll
  for (int sg = 0; sg < OpsF32::NFRAG; ++sg) a[sg] = gu[(size_t)T0 * OpsF32::TILE_FRAGS + sg * 64 + lane];
  const float* row = G.abuf + (size_t)kc * N0E_ROW + 48 * hf;
  OpsF32::Act B, Bn;
  auto load_b = [&](OpsF32::Act& X, int jj) __attribute__((always_inline)) {
    const f32x4* p = reinterpret_cast<const f32x4*>(row + (size_t)jj * KDIM);
#pragma unroll
    for (int u = 0; u < 12; ++u) { const f32x4 x = p[u]; X.v[4 * u] = x.x; X.v[4 * u + 1] = x.y; X.v[4 * u + 2] = x.z; X.v[4 * u + 3] = x.w; }
  };
  load_b(B, 0);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  // the stream's next tile after the last 0e one is the first vector tile: every prefetch is in bounds
  for (int jj = 0; jj < N0E_MIDS; ++jj) {
    load_b(Bn, jj + 1 < N0E_MIDS ? jj + 1 : jj);
    OpsF32::gemm(a, gu + (size_t)(T0 + jj + 1) * OpsF32::TILE_FRAGS, lane, B, acc);
    B = Bn;
  }
  // bias term sum_j b2_j[w] S[j], fixed order
  const float* S = G.abuf + (size_t)kc * N0E_ROW + N0E_S_OFF;
  float bs[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) bs[r] = 0.f;
  for (int jj = 0; jj < N0E_MIDS; ++jj) {
    const float sj = S[jj];
    const float* bj = bias + (size_t)(T0 + jj) * 32;
#pragma unroll
    for (int r = 0; r < 16; ++r) bs[r] = fmaf(bj[(r & 3) + 8 * (r >> 2) + 4 * hf], sj, bs[r]);
  }
  if (k < G.n_nodes) {
    float* o = G.out + (size_t)k * NS;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[(r & 3) + 8 * (r >> 2) + 4 * hf] = acc[r] + bs[r];
  }
}

hipError_t launch_node0e(const N0eArgs& a, hipStream_t s) {
  int g1 = 0, g2 = 0;
  for (int g = 0; g < a.n_groups; ++g) {
    g1 += (a.g[g].n_nodes + N0E_NPW - 1) / N0E_NPW;
    g2 += (a.g[g].n_nodes + WAVE_EDGES - 1) / WAVE_EDGES;
  }
  if (g1 == 0) return hipSuccess;
  hipLaunchKernelGGL(node0e_build_kernel, dim3(g1), dim3(64), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(node0e_gemm_kernel, dim3(g2), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace cbd
