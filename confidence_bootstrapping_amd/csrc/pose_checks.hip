// Is a sampled pose physically possible?  Four distance checks in the style of PoseBusters, for P poses of C complexes that share R
// receptors in one launch (evaluation.pose_checks_batch; the definition on the host: evaluation.pose_checks).  Per pose, over the
// ligand's pairs i < j with d = |x_i - x_j|, the ligand's triangle-smoothed bounds lower / upper and the pair's kind:
//     kind 1 (bond):      bad if d < (1 - bond_tol) lower or d > (1 + bond_tol) upper;   bond_lo = min d / lower, bond_hi = max d / upper
//     kind 2 (1-3 pair):  the same with angle_tol;                                        angle_lo, angle_hi
//     kind 0 (the rest):  a clash if d < (1 - clash_tol) lower;                           clash_ratio = min d / lower
// and over all ligand atoms i and receptor atoms a with ratio = d / (r_i + r_a):
//     a clash if ratio < rec_scale;  rec_ratio = min ratio, at (rec_lig_atom, rec_atom) -- ties to the smaller i, then the smaller a;
//     rec_dist = min d.
// One 256-thread workgroup per pose; the pose lives in LDS as [N][4] = (x, y, z, radius), 4 KB at the limit.  Pass 1: the threads stride
// over the N (N - 1) / 2 pairs, two table entries and one kind byte from global memory each.  Pass 2: the threads stride over the receptor
// atoms, one 16-byte load each, and loop over the ligand atoms in LDS (every lane reads the same address: a broadcast).  All math is fp64
// on the fp32 inputs and rounds to fp32 once.  Every output is a minimum, a maximum or an integer count: wave shuffles, then a fold over
// the four waves through LDS.  No atomics, no global scratch, no float sums: a pose's result depends neither on the order, nor on the run,
// nor on what shares the launch.
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "host_util.h"

namespace cbd {

constexpr int PC_MAX_N = 256;          // atoms of a ligand
constexpr int PC_WAVES = 4;
constexpr int PC_ROWS = 14;
// rows of the output [PC_ROWS][P]
enum { PC_BOND_LO, PC_BOND_HI, PC_ANGLE_LO, PC_ANGLE_HI, PC_CLASH_RATIO, PC_REC_RATIO, PC_REC_DIST,            // fp32
       PC_N_BOND, PC_N_ANGLE, PC_N_CLASH, PC_N_REC, PC_REC_LIG_ATOM, PC_REC_ATOM, PC_FLAGS };                   // int32
enum { PC_F_BOND = 1, PC_F_ANGLE = 2, PC_F_CLASH = 4, PC_F_REC = 8, PC_F_NO_TABLES = 16, PC_F_NO_REC = 32, PC_F_COORD = 64, PC_F_TABLE = 128 };

struct PoseChecksBatch {
  int P, C, R, max_n;
  const int* pose_cplx;            // [P] complex of the pose
  const int* pose_ptr;             // [P + 1] atoms of pos / lig_radius
  const float* pos;                // [sum N over P][3]
  const float* lig_radius;         // [sum N over P]
  const int* cplx_n;               // [C]
  const int* cplx_rec;             // [C] receptor, or -1
  const int* cplx_tab;             // [C] 0 / 1
  const int* tab_ptr;              // [C + 1] entries of bounds / kind: N * N rounded up to a multiple of four per complex with tables, else 0
  const float* bounds;             // [.][N][N]: i < j upper, j < i lower
  const unsigned char* kind;       // [.][N][N]
  const int* rec_ptr;              // [R + 1] atoms of rec
  const float4* rec;               // [sum A over R] (x, y, z, radius)
  float bond_tol, angle_tol, clash_tol, rec_scale;
  int* out;                        // [PC_ROWS][P]
};

CBD_DEV double wave_min_d(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
  return v;
}
CBD_DEV double wave_max_d(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}
CBD_DEV int wave_sum_i(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// (ratio, ligand atom, receptor atom) in lexicographic order
CBD_DEV bool pair_before(double r2, int i2, int a2, double r, int i, int a) { return r2 < r || (r2 == r && (i2 < i || (i2 == i && a2 < a))); }
CBD_DEV bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }      // false for NaN and both infinities

CBD_DEV void put_refused(const PoseChecksBatch& b, int p, int flags, bool internal, bool receptor) {
  const int nan = __float_as_int(__builtin_nanf(""));
  if (internal) {
    for (int r = PC_BOND_LO; r <= PC_CLASH_RATIO; ++r) b.out[(size_t)r * b.P + p] = nan;
    for (int r = PC_N_BOND; r <= PC_N_CLASH; ++r) b.out[(size_t)r * b.P + p] = -1;
  }
  if (receptor) {
    b.out[(size_t)PC_REC_RATIO * b.P + p] = b.out[(size_t)PC_REC_DIST * b.P + p] = nan;
    for (int r = PC_N_REC; r <= PC_REC_ATOM; ++r) b.out[(size_t)r * b.P + p] = -1;
  }
  b.out[(size_t)PC_FLAGS * b.P + p] = flags;
}

// grid: P workgroups of four waves
__global__ __launch_bounds__(256) void pose_checks_kernel(PoseChecksBatch b) {
  __shared__ float4 pose[PC_MAX_N];
  __shared__ double w_d[PC_WAVES][7];
  __shared__ int w_i[PC_WAVES][8];
  const int p = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  // the description of the pose, checked before anything is indexed with it (workgroup-uniform)
  const int c = b.pose_cplx[p];
  bool good = c >= 0 && c < b.C;
  int N = 0, a0 = 0, rec = -1, tab = 0, t0 = 0, r0 = 0, A = 0;
  if (good) {
    N = b.cplx_n[c]; rec = b.cplx_rec[c]; tab = b.cplx_tab[c];
    a0 = b.pose_ptr[p];
    good = N >= 1 && N <= b.max_n && N <= PC_MAX_N && a0 >= 0 && b.pose_ptr[p + 1] - a0 == N && rec >= -1 && rec < b.R && (tab == 0 || tab == 1);
    if (good && tab) {
      good = b.tab_ptr != nullptr && b.bounds != nullptr && b.kind != nullptr;
      if (good) {
        t0 = b.tab_ptr[c];
        good = t0 >= 0 && b.tab_ptr[c + 1] - t0 == ((N * N + 3) & ~3);
      }
    }
    if (good && rec >= 0) {
      good = b.rec_ptr != nullptr;
      if (good) {
        r0 = b.rec_ptr[rec];
        A = b.rec_ptr[rec + 1] - r0;
        good = r0 >= 0 && A >= 0 && (A == 0 || b.rec != nullptr);
      }
    }
  }
  if (!good) {   // a complex or a receptor that does not exist, sizes that contradict the pointers: NaN / -1, nothing indexed
    if (tid == 0) put_refused(b, p, PC_F_COORD, true, true);
    return;
  }
  const bool has_rec = rec >= 0 && A > 0;
  int bad_coord = 0, bad_table = 0;
  for (int i = tid; i < N; i += 256) {
    const float* __restrict__ g = b.pos + (size_t)(a0 + i) * 3;
    const float4 v = make_float4(g[0], g[1], g[2], b.lig_radius[(size_t)a0 + i]);
    if (!(finite_f(v.x) && finite_f(v.y) && finite_f(v.z))) bad_coord = 1;
    if (has_rec && !(finite_f(v.w) && v.w > 0.f)) bad_table = 1;
    pose[i] = v;
  }
  __syncthreads();

  // ---- pass 1: the ligand's own pairs, k = j (j - 1) / 2 + i for i < j
  double bond_lo = __builtin_inf(), bond_hi = -__builtin_inf(), angle_lo = __builtin_inf(), angle_hi = -__builtin_inf(), clash = __builtin_inf();
  int n_bond = 0, n_angle = 0, n_clash = 0;
  if (tab) {
    const float* __restrict__ B = b.bounds + (size_t)t0;
    const unsigned char* __restrict__ K = b.kind + (size_t)t0;
    const double bond_below = 1.0 - (double)b.bond_tol, bond_above = 1.0 + (double)b.bond_tol, angle_below = 1.0 - (double)b.angle_tol,
                 angle_above = 1.0 + (double)b.angle_tol, clash_below = 1.0 - (double)b.clash_tol;
    const int n_pairs = N * (N - 1) / 2;
    for (int k = tid; k < n_pairs; k += 256) {
      int j = (int)((1.f + sqrtf(1.f + 8.f * (float)k)) * 0.5f);
      while (j * (j - 1) / 2 > k) --j;
      while ((j + 1) * j / 2 <= k) ++j;
      const int i = k - j * (j - 1) / 2;        // 0 <= i < j < N
      const float up = B[i * N + j], lo = B[j * N + i];
      const int kd = K[i * N + j];
      if (!(finite_f(lo) && finite_f(up) && lo > 0.f && up >= lo) || kd > 2) { bad_table = 1; continue; }
      const float4 u = pose[i], v = pose[j];
      const double dx = (double)u.x - (double)v.x, dy = (double)u.y - (double)v.y, dz = (double)u.z - (double)v.z;
      const double d = sqrt(dx * dx + dy * dy + dz * dz);
      const double below = d / (double)lo, above = d / (double)up;
      if (kd == 1) {
        n_bond += (d < bond_below * (double)lo || d > bond_above * (double)up) ? 1 : 0;
        bond_lo = fmin(bond_lo, below); bond_hi = fmax(bond_hi, above);
      } else if (kd == 2) {
        n_angle += (d < angle_below * (double)lo || d > angle_above * (double)up) ? 1 : 0;
        angle_lo = fmin(angle_lo, below); angle_hi = fmax(angle_hi, above);
      } else {
        n_clash += d < clash_below * (double)lo ? 1 : 0;
        clash = fmin(clash, below);
      }
    }
  }

  // ---- pass 2: every ligand atom against every receptor atom
  double best = __builtin_inf(), near = __builtin_inf();
  int best_i = 0x7fffffff, best_a = 0x7fffffff, n_rec = 0;
  if (has_rec) {
    const float4* __restrict__ Q = b.rec + (size_t)r0;
    const double scale = (double)b.rec_scale;
    for (int a = tid; a < A; a += 256) {
      const float4 q = Q[a];
      if (!(finite_f(q.x) && finite_f(q.y) && finite_f(q.z))) bad_coord = 1;
      if (!(finite_f(q.w) && q.w > 0.f)) bad_table = 1;
      const double qx = q.x, qy = q.y, qz = q.z, qr = q.w;
      for (int i = 0; i < N; ++i) {
        const float4 u = pose[i];
        const double dx = (double)u.x - qx, dy = (double)u.y - qy, dz = (double)u.z - qz;
        const double d = sqrt(dx * dx + dy * dy + dz * dz);
        const double ratio = d / ((double)u.w + qr);
        n_rec += ratio < scale ? 1 : 0;
        near = fmin(near, d);
        if (pair_before(ratio, i, a, best, best_i, best_a)) { best = ratio; best_i = i; best_a = a; }
      }
    }
  }

  // ---- fold: lanes of a wave by shuffles, the four waves through LDS
  bond_lo = wave_min_d(bond_lo); bond_hi = wave_max_d(bond_hi); angle_lo = wave_min_d(angle_lo); angle_hi = wave_max_d(angle_hi);
  clash = wave_min_d(clash); near = wave_min_d(near);
  n_bond = wave_sum_i(n_bond); n_angle = wave_sum_i(n_angle); n_clash = wave_sum_i(n_clash); n_rec = wave_sum_i(n_rec);
  bad_coord = wave_sum_i(bad_coord); bad_table = wave_sum_i(bad_table);
  for (int off = 32; off > 0; off >>= 1) {
    const double r2 = __shfl_xor(best, off);
    const int i2 = __shfl_xor(best_i, off), a2 = __shfl_xor(best_a, off);
    if (pair_before(r2, i2, a2, best, best_i, best_a)) { best = r2; best_i = i2; best_a = a2; }
  }
  if (lane == 0) {
    w_d[wave][0] = bond_lo; w_d[wave][1] = bond_hi; w_d[wave][2] = angle_lo; w_d[wave][3] = angle_hi; w_d[wave][4] = clash;
    w_d[wave][5] = best; w_d[wave][6] = near;
    w_i[wave][0] = n_bond; w_i[wave][1] = n_angle; w_i[wave][2] = n_clash; w_i[wave][3] = n_rec; w_i[wave][4] = best_i; w_i[wave][5] = best_a;
    w_i[wave][6] = bad_coord; w_i[wave][7] = bad_table;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < PC_WAVES; ++w) {
    bond_lo = fmin(bond_lo, w_d[w][0]); bond_hi = fmax(bond_hi, w_d[w][1]); angle_lo = fmin(angle_lo, w_d[w][2]);
    angle_hi = fmax(angle_hi, w_d[w][3]); clash = fmin(clash, w_d[w][4]); near = fmin(near, w_d[w][6]);
    n_bond += w_i[w][0]; n_angle += w_i[w][1]; n_clash += w_i[w][2]; n_rec += w_i[w][3]; bad_coord += w_i[w][6]; bad_table += w_i[w][7];
    if (pair_before(w_d[w][5], w_i[w][4], w_i[w][5], best, best_i, best_a)) { best = w_d[w][5]; best_i = w_i[w][4]; best_a = w_i[w][5]; }
  }
  int flags = (tab ? 0 : PC_F_NO_TABLES) | (has_rec ? 0 : PC_F_NO_REC) | (bad_coord ? PC_F_COORD : 0) | (bad_table ? PC_F_TABLE : 0);
  if (bad_coord || bad_table) {      // a coordinate that is not finite, a malformed table entry or radius: nothing of this pose is reported
    put_refused(b, p, flags, true, true);
    return;
  }
  auto put_f = [&](int row, double v) { b.out[(size_t)row * b.P + p] = __float_as_int((float)v); };
  auto put_i = [&](int row, int v) { b.out[(size_t)row * b.P + p] = v; };
  if (tab) {
    put_f(PC_BOND_LO, bond_lo); put_f(PC_BOND_HI, bond_hi); put_f(PC_ANGLE_LO, angle_lo); put_f(PC_ANGLE_HI, angle_hi); put_f(PC_CLASH_RATIO, clash);
    put_i(PC_N_BOND, n_bond); put_i(PC_N_ANGLE, n_angle); put_i(PC_N_CLASH, n_clash);
    flags |= (n_bond ? PC_F_BOND : 0) | (n_angle ? PC_F_ANGLE : 0) | (n_clash ? PC_F_CLASH : 0);
  }
  if (has_rec) {
    put_f(PC_REC_RATIO, best); put_f(PC_REC_DIST, near);
    put_i(PC_N_REC, n_rec); put_i(PC_REC_LIG_ATOM, best_i); put_i(PC_REC_ATOM, best_a);
    flags |= n_rec ? PC_F_REC : 0;
  }
  put_refused(b, p, flags, !tab, !has_rec);      // the checks that did not run: NaN / -1; and the flags
}

}  // namespace cbd

using namespace cbd;

int cbd_pose_checks(int32_t n_poses, int32_t n_complexes, int32_t n_receptors, int32_t max_n, const int32_t* pose_cplx_dev,
                    const int32_t* pose_ptr_dev, const float* pos_dev, const float* lig_radius_dev, const int32_t* cplx_n_dev,
                    const int32_t* cplx_rec_dev, const int32_t* cplx_tab_dev, const int32_t* tab_ptr_dev, const float* bounds_dev,
                    const uint8_t* kind_dev, const int32_t* rec_ptr_dev, const float* rec_dev, float bond_tol, float angle_tol, float clash_tol,
                    float rec_scale, int32_t* out_dev, void* stream) {
  if (n_poses < 0 || n_complexes < 0 || n_receptors < 0 || max_n < 0)
    return fail(CBD_ERR_ARG, "n_poses = %d, n_complexes = %d, n_receptors = %d, max_n = %d", n_poses, n_complexes, n_receptors, max_n);
  if (max_n > PC_MAX_N)
    return fail(CBD_ERR_CAPACITY, "a ligand of %d atoms: the kernel takes up to %d (check it on the host)", max_n, PC_MAX_N);
  if (n_poses == 0) return 0;
  if (max_n < 1 || n_complexes < 1) return fail(CBD_ERR_ARG, "max_n = %d, n_complexes = %d with %d poses", max_n, n_complexes, n_poses);
  if (!(bond_tol >= 0.f && bond_tol < 1.f && angle_tol >= 0.f && angle_tol < 1.f && clash_tol >= 0.f && clash_tol < 1.f && rec_scale > 0.f &&
        rec_scale <= 3.402823466e38f))
    return fail(CBD_ERR_ARG, "thresholds bond_tol = %g, angle_tol = %g, clash_tol = %g (each in [0, 1)), rec_scale = %g (positive)", bond_tol,
                angle_tol, clash_tol, rec_scale);
  if (!pose_cplx_dev || !pose_ptr_dev || !pos_dev || !lig_radius_dev || !cplx_n_dev || !cplx_rec_dev || !cplx_tab_dev || !out_dev ||
      (n_receptors > 0 && !rec_ptr_dev))
    return fail(CBD_ERR_ARG, "null argument");
  if (reinterpret_cast<uintptr_t>(rec_dev) & 15) return fail(CBD_ERR_ARG, "rec_dev is read 16 bytes at a time and must be aligned to 16");
  const PoseChecksBatch b{n_poses, n_complexes, n_receptors, max_n, pose_cplx_dev, pose_ptr_dev, pos_dev, lig_radius_dev, cplx_n_dev, cplx_rec_dev,
                          cplx_tab_dev, tab_ptr_dev, bounds_dev, kind_dev, rec_ptr_dev, reinterpret_cast<const float4*>(rec_dev), bond_tol, angle_tol,
                          clash_tol, rec_scale, out_dev};
  hipLaunchKernelGGL(pose_checks_kernel, dim3(n_poses), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), b);
  HIPCHK(hipGetLastError());
  return 0;
}
