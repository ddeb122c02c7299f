// Ligand conformers by distance geometry (the first half of the reference's conformer matching: `generate_conformer`,
// datasets/process_mols.py:591-607, which calls rdkit's ETKDG).  The host (datasets/conformer_embedding.py) turns a molecule into lower /
// upper bounds on every pair distance [N][N] plus volume / planarity constraints on quadruples of atoms; this kernel finds coordinates
// that satisfy them, n_conformers conformers of n_mols molecules in one launch, one workgroup of 4 waves per conformer.  The route is
// rdkit's `useRandomCoords` one (no metric-matrix eigen-embedding):
//   1. random 4-D start coordinates in a box of edge 3 N^(1/3) A;
//   2. minimise  sum_{i<j} e(d_ij)  +  sum_c w_v vol_c^2  +  w_4 sum_i x_i4^2  with rdkit's distance-violation error
//        e = (d^2 / ub^2 - 1)^2 above the upper bound,  (2 lb^2 / (lb^2 + d^2) - 1)^2 below the lower,
//      vol_c = the distance of the signed volume (p1 - p0) . ((p2 - p0) x (p3 - p0)) (first three dimensions) from its allowed interval,
//      w_4 = 0.01: the fourth dimension is only weakly penalised, so a substituent on the wrong side of its centre can pass through it;
//   3. the same with w_4 = 1, w_v = 0.2, then the fourth coordinate is dropped;
//   4. a 3-D refinement with the planarity terms (the same volume of a centre and its three neighbours, or of four ring atoms, -> 0).
// Minimiser: FIRE (Bitzek et al., PRL 97, 170201) with a per-atom step clamp, a fixed iteration cap per stage, and an early exit once the
// largest force component is below CE_FTOL.  The volume intervals are narrowed by a tenth of their floor while minimising, so that a
// minimum does not sit ON the limit the acceptance test checks.
// Thread (i, s) = (tid % N, tid / N) handles atom i and every S-th partner j / constraint c, S = 256 / N; the S partial gradients of an
// atom are added in the order s = 0 .. S-1 by its owner thread, block sums are a butterfly inside each wave followed by the four waves
// in order: no atomics, every sum has a fixed order, and a conformer's result is bitwise the same whatever shares the launch.  Random
// numbers are a hash of (seed, molecule id, conformer id, atom, dimension).  Coordinates live in LDS, bounds are read from global memory
// (column i of the symmetric matrices: coalesced across the threads of a slice).
// Outputs per conformer: pos [N][3], the final error (the stage-4 objective), and ok = the acceptance test (every distance in
// [lb - tol, ub + tol], every volume inside its interval, every planarity height under its limit).
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "host_util.h"

namespace cbd {

constexpr int CE_MAX_N = 256;
constexpr int CE_MAX_CONS = 1024;
constexpr int CE_THREADS = 256;
constexpr int CE_MAX_ITERS = 100000;
constexpr float CE_FTOL = 1e-4f;
constexpr float CE_DT0 = 0.02f, CE_ALPHA0 = 0.1f, CE_MAX_STEP = 0.25f;
enum : int { CE_VOLUME = 0, CE_ABS_VOLUME = 1, CE_PLANAR = 2 };

struct EmbedArgs {
  int n_mols, n_confs, max_n, max_cons;
  const int* mol_n;          // [n_mols]
  const int* bnd_ptr;        // [n_mols + 1] prefix sums of N^2
  const float* lower;        // per molecule [N][N]
  const float* upper;
  const int* cons_ptr;       // [n_mols + 1]
  const int* cons_idx;       // [sum nc][4]
  const float* cons_lo;      // [sum nc]
  const float* cons_hi;
  const int* cons_kind;
  const int* mol_id;         // [n_mols] or null (= index): part of the random-number key
  const int* conf_mol;       // [n_confs]
  const int* conf_id;        // [n_confs]: part of the random-number key
  const int* out_ptr;        // [n_confs + 1] atoms
  unsigned long long seed;
  int iters[3];
  float bound_tol;
  float* pos_out;            // [sum N][3]
  float* err_out;            // [n_confs]
  int* ok_out;               // [n_confs]: 1 accepted, 0 not, -1 description refused
};

CBD_DEV unsigned long long ce_mix64(unsigned long long z) {   // splitmix64 finaliser (as torsion_match.hip)
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Shared {
  float4 x[CE_MAX_N];
  float4 part[CE_THREADS];
  unsigned cq[CE_MAX_CONS];       // four atom indices, one byte each (N <= 256)
  float clo[CE_MAX_CONS], chi[CE_MAX_CONS];
  unsigned char ckind[CE_MAX_CONS];
  float red[4][4];
  int flag;
};

// gradient (and energy share) of the terms thread (i, s) owns
CBD_DEV void ce_terms(const Shared& sh, int i, int s, int S, int N, int nc, const float* __restrict__ lb, const float* __restrict__ ub, float w4,
                      float wv, float wp, float4& g, float& e) {
  const float4 xi = sh.x[i];
  g = make_float4(0.f, 0.f, 0.f, 0.f);
  e = 0.f;
  for (int j = s; j < N; j += S) {
    if (j == i) continue;
    const float4 xj = sh.x[j];
    const float l = lb[(size_t)j * N + i], u = ub[(size_t)j * N + i];
    const float dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z, dw = xi.w - xj.w;
    const float d2 = dx * dx + dy * dy + dz * dz + dw * dw;
    const float u2 = u * u, l2 = l * l;
    float coef = 0.f;
    if (d2 > u2 && u2 > 0.f) {
      const float t = d2 / u2 - 1.f;
      e += 0.5f * t * t;            // a pair is seen from both of its atoms
      coef = 4.f * t / u2;
    } else if (d2 < l2) {
      const float den = l2 + d2, t = 2.f * l2 / den - 1.f;
      e += 0.5f * t * t;
      coef = -8.f * t * l2 / (den * den);
    }
    g.x += coef * dx; g.y += coef * dy; g.z += coef * dz; g.w += coef * dw;
  }
  if (s == 0) {
    e += w4 * xi.w * xi.w;
    g.w += 2.f * w4 * xi.w;
  }
  for (int c = s; c < nc; c += S) {
    const unsigned q = sh.cq[c];
    const int i0 = q & 255u, i1 = (q >> 8) & 255u, i2 = (q >> 16) & 255u, i3 = q >> 24;
    if (i != i0 && i != i1 && i != i2 && i != i3) continue;
    const float4 p0 = sh.x[i0], p1 = sh.x[i1], p2 = sh.x[i2], p3 = sh.x[i3];
    const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z;
    const float bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
    const float cx = p3.x - p0.x, cy = p3.y - p0.y, cz = p3.z - p0.z;
    const float bcx = by * cz - bz * cy, bcy = bz * cx - bx * cz, bcz = bx * cy - by * cx;
    const float V = ax * bcx + ay * bcy + az * bcz;
    const int kind = sh.ckind[c];
    float r, w, sg = 1.f;
    if (kind == CE_PLANAR) {
      r = V; w = wp;
    } else {
      if (kind == CE_ABS_VOLUME && V < 0.f) sg = -1.f;
      const float lo = sh.clo[c], hi = sh.chi[c], m = 0.1f * fminf(fabsf(lo), fabsf(hi));
      const float Ve = sg * V;
      r = Ve < lo + m ? Ve - (lo + m) : (Ve > hi - m ? Ve - (hi - m) : 0.f);
      w = wv;
    }
    if (i == i0) e += w * r * r;
    const float f = 2.f * w * r * sg;
    if (f != 0.f) {
      const float cax = cy * az - cz * ay, cay = cz * ax - cx * az, caz = cx * ay - cy * ax;
      const float abx = ay * bz - az * by, aby = az * bx - ax * bz, abz = ax * by - ay * bx;
      float gx, gy, gz;
      if (i == i1) { gx = bcx; gy = bcy; gz = bcz; }
      else if (i == i2) { gx = cax; gy = cay; gz = caz; }
      else if (i == i3) { gx = abx; gy = aby; gz = abz; }
      else { gx = -(bcx + cax + abx); gy = -(bcy + cay + aby); gz = -(bcz + caz + abz); }
      g.x += f * gx; g.y += f * gy; g.z += f * gz;
    }
  }
}

// sums of a, b, c and the maximum of m over the workgroup, the same value in every thread; two barriers
CBD_DEV void ce_block_reduce(Shared& sh, float& a, float& b, float& c, float& m) {
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off); b += __shfl_xor(b, off); c += __shfl_xor(c, off);
    m = fmaxf(m, __shfl_xor(m, off));
  }
  const int wave = threadIdx.x >> 6;
  if (lane_id() == 0) { sh.red[wave][0] = a; sh.red[wave][1] = b; sh.red[wave][2] = c; sh.red[wave][3] = m; }
  __syncthreads();
  a = ((sh.red[0][0] + sh.red[1][0]) + sh.red[2][0]) + sh.red[3][0];
  b = ((sh.red[0][1] + sh.red[1][1]) + sh.red[2][1]) + sh.red[3][1];
  c = ((sh.red[0][2] + sh.red[1][2]) + sh.red[2][2]) + sh.red[3][2];
  m = fmaxf(fmaxf(sh.red[0][3], sh.red[1][3]), fmaxf(sh.red[2][3], sh.red[3][3]));
  __syncthreads();
}

// one FIRE minimisation; x is the owner thread's (tid < N) copy of sh.x[tid]
CBD_DEV void ce_minimise(Shared& sh, int N, int nc, int S, const float* lb, const float* ub, float w4, float wv, float wp, float dtmax, int cap,
                         float4& x) {
  const int tid = threadIdx.x, i = tid % N, s = tid / N;
  const bool active = s < S, owner = tid < N;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  float dt = CE_DT0, alpha = CE_ALPHA0;
  int npos = 0;
  for (int it = 0; it < cap; ++it) {
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    float e = 0.f;
    if (active) ce_terms(sh, i, s, S, N, nc, lb, ub, w4, wv, wp, g, e);
    sh.part[tid] = g;
    __syncthreads();
    float4 F = make_float4(0.f, 0.f, 0.f, 0.f);
    float p = 0.f, ff = 0.f, vv = 0.f, fm = 0.f;
    if (owner) {
      for (int q = 0; q < S; ++q) {
        const float4 t = sh.part[tid + q * N];
        F.x -= t.x; F.y -= t.y; F.z -= t.z; F.w -= t.w;
      }
      v.x += dt * F.x; v.y += dt * F.y; v.z += dt * F.z; v.w += dt * F.w;
      p = F.x * v.x + F.y * v.y + F.z * v.z + F.w * v.w;
      ff = F.x * F.x + F.y * F.y + F.z * F.z + F.w * F.w;
      vv = v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
      fm = fmaxf(fmaxf(fabsf(F.x), fabsf(F.y)), fmaxf(fabsf(F.z), fabsf(F.w)));
    }
    ce_block_reduce(sh, p, ff, vv, fm);
    if (!(fm >= CE_FTOL)) break;          // converged (or not a number): uniform over the workgroup
    if (p > 0.f) {
      const float k = alpha * sqrtf(vv) / fmaxf(sqrtf(ff), 1e-30f);
      v.x = (1.f - alpha) * v.x + k * F.x; v.y = (1.f - alpha) * v.y + k * F.y;
      v.z = (1.f - alpha) * v.z + k * F.z; v.w = (1.f - alpha) * v.w + k * F.w;
      if (++npos > 5) { dt = fminf(dt * 1.1f, dtmax); alpha *= 0.99f; }
    } else {
      v = make_float4(0.f, 0.f, 0.f, 0.f);
      npos = 0; dt *= 0.5f; alpha = CE_ALPHA0;
    }
    if (owner) {
      float dx = dt * v.x, dy = dt * v.y, dz = dt * v.z, dw = dt * v.w;
      const float n = sqrtf(dx * dx + dy * dy + dz * dz + dw * dw);
      const float sc = fminf(1.f, CE_MAX_STEP / fmaxf(n, 1e-30f));
      v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
      x.x += dx * sc; x.y += dy * sc; x.z += dz * sc; x.w += dw * sc;
      sh.x[tid] = x;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(CE_THREADS) void embed_conformers_kernel(EmbedArgs a) {
  __shared__ Shared sh;
  const int cf = blockIdx.x, tid = threadIdx.x;
  // ---- the description is checked before anything is indexed with it
  const int m = a.conf_mol[cf];
  bool good = m >= 0 && m < a.n_mols;
  int N = 0, nc = 0, b0 = 0, c0 = 0, o0 = 0;
  if (good) {
    N = a.mol_n[m];
    b0 = a.bnd_ptr[m]; c0 = a.cons_ptr[m]; o0 = a.out_ptr[cf];
    nc = a.cons_ptr[m + 1] - c0;
    good = N >= 1 && N <= a.max_n && N <= CE_MAX_N && b0 >= 0 && (long long)a.bnd_ptr[m + 1] - b0 == (long long)N * N && c0 >= 0 && nc >= 0 &&
           nc <= a.max_cons && nc <= CE_MAX_CONS && o0 >= 0 && a.out_ptr[cf + 1] - o0 == N;
  }
  if (tid == 0) sh.flag = 0;
  __syncthreads();
  if (good) {
    bool bad = false;
    for (int c = tid; c < nc; c += CE_THREADS) {
      const int* q = a.cons_idx + (size_t)(c0 + c) * 4;
      const int i0 = q[0], i1 = q[1], i2 = q[2], i3 = q[3], kind = a.cons_kind[c0 + c];
      const bool okc = i0 >= 0 && i0 < N && i1 >= 0 && i1 < N && i2 >= 0 && i2 < N && i3 >= 0 && i3 < N && i0 != i1 && i0 != i2 && i0 != i3 &&
                       i1 != i2 && i1 != i3 && i2 != i3 && kind >= CE_VOLUME && kind <= CE_PLANAR;
      bad = bad || !okc;
      sh.cq[c] = okc ? ((unsigned)i0 | ((unsigned)i1 << 8) | ((unsigned)i2 << 16) | ((unsigned)i3 << 24)) : 0u;
      sh.clo[c] = a.cons_lo[c0 + c]; sh.chi[c] = a.cons_hi[c0 + c];
      sh.ckind[c] = (unsigned char)(okc ? kind : 0);
    }
    if (bad) sh.flag = 1;       // every writer stores the same value
  }
  __syncthreads();
  if (!good || sh.flag) {       // uniform: refused, the coordinates are left as they were
    if (tid == 0) { a.err_out[cf] = __builtin_nanf(""); a.ok_out[cf] = -1; }
    return;
  }
  const float* __restrict__ lb = a.lower + b0;
  const float* __restrict__ ub = a.upper + b0;
  const int S = CE_THREADS / N;
  // ---- 1. random 4-D start
  float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
  if (tid < N) {
    const unsigned long long key_m = ce_mix64(ce_mix64(a.seed) ^ (unsigned long long)(unsigned)(a.mol_id ? a.mol_id[m] : m));
    const unsigned long long key = ce_mix64(key_m ^ ((unsigned long long)(unsigned)a.conf_id[cf] << 32));
    const float box = 3.f * cbrtf((float)N);
    float u[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
      u[d] = (float)(ce_mix64(key ^ (((unsigned long long)tid << 8) | (unsigned)d)) >> 40) * (1.0f / 16777216.0f) - 0.5f;
    x = make_float4(u[0] * box, u[1] * box, u[2] * box, u[3] * box);
    sh.x[tid] = x;
  }
  __syncthreads();
  // ---- 2. / 3. 4-D, the fourth dimension weakly then strongly penalised
  ce_minimise(sh, N, nc, S, lb, ub, 0.01f, 1.0f, 0.f, 0.2f, a.iters[0], x);
  ce_minimise(sh, N, nc, S, lb, ub, 1.0f, 0.2f, 0.f, 0.2f, a.iters[1], x);
  if (tid < N) { x.w = 0.f; sh.x[tid] = x; }
  __syncthreads();
  // ---- 4. 3-D with the planarity terms (stiffer: a smaller largest time step)
  ce_minimise(sh, N, nc, S, lb, ub, 0.f, 1.0f, 1.0f, 0.05f, a.iters[2], x);
  // ---- error and acceptance
  const int i = tid % N, s = tid / N;
  float4 g;
  float e = 0.f;
  bool bad = false;
  if (s < S) {
    ce_terms(sh, i, s, S, N, nc, lb, ub, 0.f, 1.0f, 1.0f, g, e);
    const float4 xi = sh.x[i];
    for (int j = s; j < N; j += S) {
      if (j == i) continue;
      const float4 xj = sh.x[j];
      const float dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
      const float d = sqrtf(dx * dx + dy * dy + dz * dz);
      bad = bad || !(d >= lb[(size_t)j * N + i] - a.bound_tol && d <= ub[(size_t)j * N + i] + a.bound_tol);
    }
    for (int c = s; c < nc; c += S) {
      const unsigned q = sh.cq[c];
      if (i != (int)(q & 255u)) continue;
      const float4 p0 = sh.x[i], p1 = sh.x[(q >> 8) & 255u], p2 = sh.x[(q >> 16) & 255u], p3 = sh.x[q >> 24];
      const int kind = sh.ckind[c];
      if (kind == CE_PLANAR) {   // height of p0 over the plane through p1, p2, p3
        const float bx = p2.x - p1.x, by = p2.y - p1.y, bz = p2.z - p1.z, cx = p3.x - p1.x, cy = p3.y - p1.y, cz = p3.z - p1.z;
        const float nx = by * cz - bz * cy, ny = bz * cx - bx * cz, nz = bx * cy - by * cx;
        const float h = fabsf((p0.x - p1.x) * nx + (p0.y - p1.y) * ny + (p0.z - p1.z) * nz) / fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), 1e-12f);
        bad = bad || !(h <= sh.chi[c]);
      } else {
        const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z, bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
        const float cx = p3.x - p0.x, cy = p3.y - p0.y, cz = p3.z - p0.z;
        float V = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
        if (kind == CE_ABS_VOLUME) V = fabsf(V);
        bad = bad || !(V >= sh.clo[c] && V <= sh.chi[c]);
      }
    }
  }
  float e1 = e, z0 = 0.f, z1 = 0.f, badf = bad ? 1.f : 0.f;
  ce_block_reduce(sh, e1, z0, z1, badf);
  if (tid < N) {
    float* O = a.pos_out + (size_t)(o0 + tid) * 3;
    O[0] = x.x; O[1] = x.y; O[2] = x.z;
  }
  if (tid == 0) { a.err_out[cf] = e1; a.ok_out[cf] = badf > 0.f ? 0 : 1; }
}

}  // namespace cbd

using namespace cbd;

int cbd_embed_conformers(int32_t n_mols, int32_t n_conformers, int32_t max_n, int32_t max_constraints, const int32_t* mol_n_dev,
                         const int32_t* bnd_ptr_dev, const float* lower_dev, const float* upper_dev, const int32_t* cons_ptr_dev,
                         const int32_t* cons_idx_dev, const float* cons_lo_dev, const float* cons_hi_dev, const int32_t* cons_kind_dev,
                         const int32_t* mol_id_dev, const int32_t* conf_mol_dev, const int32_t* conf_id_dev, const int32_t* out_ptr_dev,
                         uint64_t seed, int32_t iters_4d_weak, int32_t iters_4d_strong, int32_t iters_3d, float bound_tol, float* pos_out_dev,
                         float* err_out_dev, int32_t* ok_out_dev, void* stream) {
  if (n_mols < 0 || n_conformers < 0 || max_n < 1 || max_constraints < 0) return fail(CBD_ERR_ARG, "bad size argument");
  if (max_n > CE_MAX_N) return fail(CBD_ERR_CAPACITY, "N = %d atoms exceeds the capacity %d", max_n, CE_MAX_N);
  if (max_constraints > CE_MAX_CONS) return fail(CBD_ERR_CAPACITY, "%d constraints exceed the capacity %d", max_constraints, CE_MAX_CONS);
  if (iters_4d_weak < 0 || iters_4d_strong < 0 || iters_3d < 0 || iters_4d_weak > CE_MAX_ITERS || iters_4d_strong > CE_MAX_ITERS ||
      iters_3d > CE_MAX_ITERS)
    return fail(CBD_ERR_ARG, "iteration cap outside 0..%d", CE_MAX_ITERS);
  if (!(bound_tol >= 0.f)) return fail(CBD_ERR_ARG, "bound_tol = %g", (double)bound_tol);
  if (n_conformers == 0) return 0;
  if (n_mols == 0) return fail(CBD_ERR_ARG, "conformers of no molecule");
  if (!mol_n_dev || !bnd_ptr_dev || !lower_dev || !upper_dev || !cons_ptr_dev || !conf_mol_dev || !conf_id_dev || !out_ptr_dev || !pos_out_dev ||
      !err_out_dev || !ok_out_dev)
    return fail(CBD_ERR_ARG, "null argument");
  if (max_constraints > 0 && (!cons_idx_dev || !cons_lo_dev || !cons_hi_dev || !cons_kind_dev)) return fail(CBD_ERR_ARG, "null constraint array");
  const EmbedArgs args{n_mols, n_conformers, max_n, max_constraints, mol_n_dev, bnd_ptr_dev, lower_dev, upper_dev, cons_ptr_dev, cons_idx_dev,
                       cons_lo_dev, cons_hi_dev, cons_kind_dev, mol_id_dev, conf_mol_dev, conf_id_dev, out_ptr_dev, (unsigned long long)seed,
                       {iters_4d_weak, iters_4d_strong, iters_3d}, bound_tol, pos_out_dev, err_out_dev, ok_out_dev};
  hipLaunchKernelGGL(embed_conformers_kernel, dim3(n_conformers), dim3(CE_THREADS), 0, reinterpret_cast<hipStream_t>(stream), args);
  HIPCHK(hipGetLastError());
  return 0;
}
