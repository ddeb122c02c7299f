// Device pieces of graph construction and edge featurisation that the score engine (kernels.hip) and the all-atom confidence
// engine (conf_kernels.hip) both run: the kernels that decide which edges exist have ONE body, so a test of either engine
// tests both.  64-wide wavefronts, one wave per aggregating node; COUNT pass (FILL = false), scan, FILL pass.
#pragma once
#include "common.h"
#include "device_util.h"

namespace cbd {

// where the FILL pass of an edge group writes (the same arrays under both engines' field names); bond4 / pair: null if the group has none
struct EdgeOut {
  int *src, *dst, *aidx;
  float *vec, *dist, *bond4;
  int* pair;   // [aggregating node][n candidates] edge id of the pair or -1
};

CBD_DEV void put_edge(const EdgeOut& o, int e, int src, int dst, float dx, float dy, float dz) {
  float ux, uy, uz, n;
  unit_vec(dx, dy, dz, ux, uy, uz, n);
  o.src[e] = src; o.dst[e] = dst; o.aidx[e] = e;
  reinterpret_cast<f32x4*>(o.vec)[e] = f32x4{ux, uy, uz, 0.f};
  o.dist[e] = n;
}

// Ligand-ligand edges aggregated by atom `a` at (px, py, pz) of the pose whose coordinates are P (node = joint index of a, node0 = of the
// pose's atom 0): bonds first, then radius-graph edges (score_model.py:502-507, all_atom_score_model.py:530-553).  Returns the edge count.
// radius_graph(pos, r, batch) returns [neighbour; centre] rows and the layer aggregates into row 0: node a receives an edge from
// every centre y that has a among the first lig_cap+1 in-radius atoms of ITS scan (index order, self included, torch_cluster
// radius with max_num_neighbors+1).  rank_y(a) = #{x < a : |x - y| < r}.
template <bool FILL>
CBD_DEV int ligand_ligand_edges(const float* P, int Nl, int a, float px, float py, float pz, int node, int node0, const int* bond_row,
                                const int* bond_dst, const float* bond_attr, const int* start, float lig_r2, int lig_cap, int lane,
                                const EdgeOut& o) {
  const int nb0 = bond_row[a], nb1 = bond_row[a + 1];
  int base = 0;
  if (FILL) {
    base = start[node];
    for (int k = nb0 + lane; k < nb1; k += 64) {
      const int e = base + (k - nb0), d = bond_dst[k];
      put_edge(o, e, node, node0 + d, P[3 * d] - px, P[3 * d + 1] - py, P[3 * d + 2] - pz);
      reinterpret_cast<f32x4*>(o.bond4)[e] = reinterpret_cast<const f32x4*>(bond_attr)[k];
    }
    base += nb1 - nb0;
  }
  int kept = 0;
  for (int c0 = 0; c0 < Nl; c0 += 64) {
    const int d = c0 + lane;   // candidate centre y
    bool keep = false;
    if (d < Nl && d != a) {
      const float yx = P[3 * d], yy = P[3 * d + 1], yz = P[3 * d + 2];
      if (dist2_nofma(px, py, pz, yx, yy, yz) < lig_r2) {
        int rank = 0;
        for (int x = 0; x < a; ++x) rank += dist2_nofma(P[3 * x], P[3 * x + 1], P[3 * x + 2], yx, yy, yz) < lig_r2 ? 1 : 0;
        keep = rank < lig_cap + 1;
      }
    }
    const unsigned long long mk = __ballot(keep);
    if (FILL && keep) {
      const int e = base + kept + popc_below(mk, lane);
      put_edge(o, e, node, node0 + d, P[3 * d] - px, P[3 * d + 1] - py, P[3 * d + 2] - pz);
      reinterpret_cast<f32x4*>(o.bond4)[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    kept += __popcll(mk);
  }
  return (nb1 - nb0) + kept;
}

// Ligand -> receptor-node cross edges of the atom at (px, py, pz): radius on cutoff-scaled coordinates (score_model.py:564-573,
// all_atom_score_model.py:590-597; the cap of 10000 never binds for Nr <= 10000) over the residues `kept` admits, plus the
// (atom, residue) -> edge id map the flipped edges are built from.  rec0 = joint index of the pose's residue 0.
struct AllResidues { CBD_DEV bool operator()(int) const { return true; } };
template <bool FILL, class Kept>
CBD_DEV int ligand_receptor_edges(float px, float py, float pz, const float* rec_pos, int Nr, float cutoff, Kept kept, int node, int rec0,
                                  const int* start, int lane, const EdgeOut& o) {
  const float lp[3] = {px, py, pz};
  int n_e = 0;
  const int base = FILL ? start[node] : 0;
  for (int c0 = 0; c0 < Nr; c0 += 64) {
    const int r = c0 + lane;
    bool in = false;
    if (r < Nr) in = kept(r) && cross_pair_in(lp, rec_pos + 3 * r, cutoff);
    const unsigned long long m = __ballot(in);
    if (FILL && r < Nr) {
      int eid = -1;
      if (in) {
        eid = base + n_e + popc_below(m, lane);
        put_edge(o, eid, node, rec0 + r, rec_pos[3 * r] - px, rec_pos[3 * r + 1] - py, rec_pos[3 * r + 2] - pz);
      }
      o.pair[(size_t)node * Nr + r] = eid;
    }
    n_e += __popcll(m);
  }
  return n_e;
}

// Flipped cross edges of the score engine, aggregated by residue r (joint index rec_node) of the pose with coordinates P and
// ligand nodes from lig0 on: the same pair test from the other side (score_model.py:356-357); the FILL pass reads the edge ids
// and unit vectors the ligand side wrote.  o.pair / lr_vec: the ligand -> receptor map and vectors.
template <bool FILL>
CBD_DEV int receptor_ligand_edges(const float* P, int Nl, const float* rec_pos, int Nr, int r, float cutoff, int rec_node, int lig0,
                                  int base, const float* lr_vec, int lane, const EdgeOut& o) {
  const float* rp = rec_pos + 3 * r;
  int nrl = 0;
  for (int c0 = 0; c0 < Nl; c0 += 64) {
    const int a = c0 + lane;
    bool in = false;
    if (a < Nl) in = cross_pair_in(P + 3 * a, rp, cutoff);
    const unsigned long long m = __ballot(in);
    if (FILL && in) {
      const int e = base + nrl + popc_below(m, lane);
      const int lr = o.pair[(size_t)(lig0 + a) * Nr + r];
      const f32x4 vv = reinterpret_cast<const f32x4*>(lr_vec)[lr];
      o.src[e] = rec_node; o.dst[e] = lig0 + a; o.aidx[e] = lr;
      reinterpret_cast<f32x4*>(o.vec)[e] = f32x4{-vv.x, -vv.y, -vv.z, 0.f};   // sh(-edge_vec), score_model.py:582
    }
    nrl += __popcll(m);
  }
  return nrl;
}

// Exclusive scan start[i] = sum of cnt[0 .. i) by ONE 1024-thread workgroup (wave-shuffle scan over coalesced 1024-entry
// chunks); returns the total to every thread.
CBD_DEV int block_exclusive_scan(const int* cnt, int* start, int n) {
  __shared__ int wsum[16];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int i = base + tid;
    const int v = i < n ? cnt[i] : 0;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int y = __shfl_up(x, off, 64);
      if (lane >= off) x += y;
    }
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wid; ++w) woff += wsum[w];
    const int carry = carry_s;
    if (i < n) start[i] = carry + woff + x - v;
    __syncthreads();
    if (tid == 1023) carry_s = carry + woff + x;
    __syncthreads();
  }
  return carry_s;
}

// Edge embedding MLP of one edge (GaussianSmearing + Linear / ReLU / Linear, EdgeMlp of common.h), NS wide: all weight addresses are
// wave-uniform (scalar loads), the products are straight-line FMAs on register arrays, the lane writes its own row.
template <int NS_>
CBD_DEV void edge_mlp_row(const EdgeMlp& m, const float* __restrict__ dist, const float* __restrict__ bond4, float* __restrict__ out, int e) {
  const float d = dist[e];
  float h[NS_];
#pragma unroll
  for (int o = 0; o < NS_; ++o) h[o] = m.part[o];
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const float t = d - m.offset[k];
    const float gk = expf(m.coeff * (t * t));
#pragma unroll
    for (int o = 0; o < NS_; ++o) h[o] = fmaf(m.WgT[k * NS_ + o], gk, h[o]);
  }
  if (m.WbT && bond4) {
    const f32x4 b = reinterpret_cast<const f32x4*>(bond4)[e];
    const float bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int o = 0; o < NS_; ++o) h[o] = fmaf(m.WbT[c * NS_ + o], bb[c], h[o]);
  }
  float r[NS_];
#pragma unroll
  for (int o = 0; o < NS_; ++o) { h[o] = fmaxf(h[o], 0.f); r[o] = m.b1[o]; }
#pragma unroll
  for (int k = 0; k < NS_; ++k)
#pragma unroll
    for (int o = 0; o < NS_; ++o) r[o] = fmaf(m.W1T[k * NS_ + o], h[k], r[o]);
  f32x4* po = reinterpret_cast<f32x4*>(out + (size_t)e * NS_);
#pragma unroll
  for (int q = 0; q < NS_ / 4; ++q) po[q] = f32x4{r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]};
}

}  // namespace cbd
