// Distinct binding modes among the sampled poses of G complexes in one call (evaluation.cluster_poses_batch; host restatement:
// evaluation.cluster_poses).  Two kernels behind each other on the caller's stream:
//   pose_pair_kernel   D[i][j] = float(sqrt(min_k S(i, j, k) / N)),  S(i, j, k) = sum_a |x_i[idx_ref[k][a]] - x_j[idx_pos[k][a]]|^2  for i < j,
//                      the expression of pose_metrics_kernel (pose_metrics.hip) with pose i in the place of the crystal pose: fp64 sums on
//                      the fp32 coordinates.  D[j][i] is written from the same value, the diagonal is 0.
//   pose_mode_kernel   leader clustering in rank order on that matrix: pose p joins the best-ranked head h with D[h][p] <= cutoff, else it
//                      becomes a head.  Only heads are compared against.
// Pair kernel: grid (tile pairs, G).  One 256-thread workgroup per pair of 8-pose tiles (ti <= tj) of one group; both tiles live in LDS
// atom-major ([atom][8 poses][3]: the eight poses a wave reads for one atom lie in 24 consecutive words, no bank is hit twice).  One lane
// per pose pair of the tile (i = lane / 8, j = lane % 8); on the diagonal tile only the i <= j lanes write.  The four waves deal the
// isomorphisms among themselves (k = w, w + 4, ...); inside a wave k and a are uniform, so the index tables are read once per wave -- 64
// entries in one coalesced load, each handed to the 64 pairs as a scalar (v_readlane) -- where the per-pose kernel reads them per pose.
// Each lane adds a = 0 .. N-1 in order, keeps its minimum over its k, and the four minima are folded through LDS: a minimum does not
// depend on the order.  No atomics, no global scratch: a group's result is bitwise the same alone or inside any batch.
// Every workgroup of a group walks the whole of both index tables, so each of them sees an entry outside [0, N) and writes NaN for its
// own tile; the (0, 0) workgroup leaves n_modes = -1 (refused) or 0 for the mode kernel, which overwrites it.
#include <atomic>

#include <hip/hip_runtime.h>

#include "device_util.h"
#include "host_util.h"

namespace cbd {

constexpr int PC_MAX_N = 512;          // atoms of a ligand: 2 tiles * 8 poses * 512 atoms * 12 B = 96 KB of LDS at the limit
constexpr int PC_MAX_P = 256;          // poses of a group
constexpr int PC_TILE = 8;
constexpr int PC_WAVES = 4;

struct PoseModesBatch {
  int G, max_n, max_p, n_poses, n_atoms, n_matrix;
  const int* grp_n;                // [G]
  const int* grp_p;                // [G]
  const int* grp_k;                // [G]
  const double* grp_cutoff;        // [G]
  const int* pose_ptr;             // [G + 1] poses
  const int* atom_ptr;             // [G + 1] atoms of pos (P * N per group)
  const int* mat_ptr;              // [G + 1] elements of matrix (P * P per group)
  const float* pos;                // [sum P N][3]
  const int* const* idx_ref;       // [G] -> [K][N]
  const int* const* idx_pos;       // [G] -> [K][N]
  float* matrix;                   // [sum P P]
  int* head;                       // [sum P]
  int* mode;                       // [sum P]
  int* n_modes;                    // [G]
};

struct PoseGroup {
  int N, P, K, p0, a0, m0;
  const int* IR;
  const int* IP;
};

// the description of a group, checked before anything is indexed with it
CBD_DEV bool read_group(const PoseModesBatch& b, int g, PoseGroup& q) {
  q.N = b.grp_n[g]; q.P = b.grp_p[g]; q.K = b.grp_k[g];
  q.p0 = b.pose_ptr[g]; q.a0 = b.atom_ptr[g]; q.m0 = b.mat_ptr[g];
  q.IR = b.idx_ref[g]; q.IP = b.idx_pos[g];
  if (!(q.N >= 1 && q.N <= b.max_n && q.P >= 1 && q.P <= b.max_p && q.K >= 1 && q.IR != nullptr && q.IP != nullptr)) return false;
  const long long P = q.P, N = q.N;
  return q.p0 >= 0 && (long long)b.pose_ptr[g + 1] - q.p0 == P && q.p0 + P <= b.n_poses &&
         q.a0 >= 0 && (long long)b.atom_ptr[g + 1] - q.a0 == P * N && q.a0 + P * N <= b.n_atoms &&
         q.m0 >= 0 && (long long)b.mat_ptr[g + 1] - q.m0 == P * P && q.m0 + P * P <= b.n_matrix;
}

// `np` poses [np][N][3] of global memory into a tile [N][8][3]; fin[s] = 0 for a pose with a coordinate that is not finite
CBD_DEV void load_tile(float* __restrict__ tile, int* fin, const float* __restrict__ gp, int np, int N, int tid) {
  const int per = 3 * N;
  for (int e = tid; e < np * per; e += 64 * PC_WAVES) {
    const int s = e / per, r = e - s * per, a = r / 3, c = r - 3 * a;
    const float v = gp[e];
    tile[(a * PC_TILE + s) * 3 + c] = v;
    if (!(fabsf(v) <= 3.402823466e38f)) fin[s] = 0;      // several threads may store the same 0
  }
}

// grid: (T (T + 1) / 2 with T = ceil(max_p / 8), G) workgroups of four waves; dynamic LDS: 2 * max_n * 8 * 3 floats
__global__ __launch_bounds__(64 * PC_WAVES) void pose_pair_kernel(PoseModesBatch b) {
  extern __shared__ float tiles[];   // tile ti [max_n][8][3], then tile tj
  __shared__ double w_s[PC_WAVES][64];
  __shared__ int fin[2 * PC_TILE];
  const int g = blockIdx.y, tid = threadIdx.x, lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  PoseGroup q;
  if (!read_group(b, g, q)) return;   // the mode kernel reports it; nothing is indexed
  const int N = q.N, P = q.P, K = q.K;
  const int T = (P + PC_TILE - 1) / PC_TILE;
  int t = blockIdx.x, ti = 0;          // row ti of the upper triangle of tile pairs holds T - ti of them
  while (ti < T && t >= T - ti) { t -= T - ti; ++ti; }
  if (ti >= T) return;                 // the grid is sized for the largest group of the launch
  const int tj = ti + t;
  const bool diag = ti == tj;
  float* __restrict__ A = tiles;
  float* __restrict__ B = diag ? tiles : tiles + (size_t)b.max_n * PC_TILE * 3;
  if (tid < 2 * PC_TILE) fin[tid] = 1;
  __syncthreads();
  const float* __restrict__ gp = b.pos + (size_t)q.a0 * 3;
  load_tile(A, fin, gp + (size_t)ti * PC_TILE * N * 3, min(PC_TILE, P - ti * PC_TILE), N, tid);
  if (!diag) load_tile(B, fin + PC_TILE, gp + (size_t)tj * PC_TILE * N * 3, min(PC_TILE, P - tj * PC_TILE), N, tid);
  __syncthreads();

  // a slot past the group's last pose holds whatever LDS held: its lanes compute on it and write nothing
  const int li = lane >> 3, lj = lane & 7;
  const float* __restrict__ xi = A + li * 3;
  const float* __restrict__ xj = B + lj * 3;
  const int* __restrict__ IR = q.IR;
  const int* __restrict__ IP = q.IP;
  bool in = true;                      // every index this lane read named an atom
  double best = __builtin_inf();
  for (int k = wave; k < K; k += PC_WAVES) {
    const int* __restrict__ ir = IR + (size_t)k * N;
    const int* __restrict__ ip = IP + (size_t)k * N;
    double s = 0.0;
    for (int a0 = 0; a0 < N; a0 += 64) {
      // 64 entries of both tables in one coalesced read, lane l holding atom a0 + l; each is then handed to all 64 pairs as a scalar
      const int mine = a0 + lane;
      int rv = mine < N ? ir[mine] : 0, pv = mine < N ? ip[mine] : 0;
      if ((unsigned)rv >= (unsigned)N || (unsigned)pv >= (unsigned)N) { in = false; rv = 0; pv = 0; }   // reported below; LDS is not indexed with it
      const int cnt = min(64, N - a0);
      for (int t = 0; t < cnt; ++t) {
        const int r = __builtin_amdgcn_readlane(rv, t), p = __builtin_amdgcn_readlane(pv, t);
        const float* __restrict__ u = xi + r * (PC_TILE * 3);
        const float* __restrict__ v = xj + p * (PC_TILE * 3);
        const double dx = (double)u[0] - (double)v[0], dy = (double)u[1] - (double)v[1], dz = (double)u[2] - (double)v[2];
        s += dx * dx + dy * dy + dz * dz;
      }
    }
    best = fmin(best, s);
  }
  w_s[wave][lane] = best;
  const bool bad = __syncthreads_or(in ? 0 : 1) != 0;   // also orders w_s
  if (tid < 64) {
    for (int w = 1; w < PC_WAVES; ++w) best = fmin(best, w_s[w][lane]);
    const int i = ti * PC_TILE + li, j = tj * PC_TILE + lj;
    if (i < P && j < P && (!diag || li <= lj)) {
      const bool finite = fin[li] != 0 && fin[(diag ? 0 : PC_TILE) + lj] != 0;
      const float d = bad || !finite ? __builtin_nanf("") : i == j ? 0.f : (float)sqrt(best / (double)N);
      float* __restrict__ D = b.matrix + q.m0;
      D[(size_t)i * P + j] = d;
      D[(size_t)j * P + i] = d;
    }
    if (ti == 0 && tj == 0 && tid == 0) b.n_modes[g] = bad ? -1 : 0;
  }
}

// grid: G workgroups of one wave, behind pose_pair_kernel on the same stream
__global__ __launch_bounds__(64) void pose_mode_kernel(PoseModesBatch b) {
  __shared__ int heads[PC_MAX_P];
  const int g = blockIdx.x, lane = threadIdx.x;
  PoseGroup q;
  if (!read_group(b, g, q)) {
    // sizes that contradict each other or the launch, no index table: -1 / NaN over the extents the prefix arrays give, where those lie
    // inside the outputs; nothing else is indexed
    const long long p0 = b.pose_ptr[g], p1 = b.pose_ptr[g + 1], m0 = b.mat_ptr[g], m1 = b.mat_ptr[g + 1];
    if (p0 >= 0 && p0 <= p1 && p1 <= b.n_poses)
      for (long long p = p0 + lane; p < p1; p += 64) b.head[p] = b.mode[p] = -1;
    if (m0 >= 0 && m0 <= m1 && m1 <= b.n_matrix)
      for (long long m = m0 + lane; m < m1; m += 64) b.matrix[m] = __builtin_nanf("");
    if (lane == 0) b.n_modes[g] = -1;
    return;
  }
  const int P = q.P;
  int* __restrict__ head = b.head + q.p0;
  int* __restrict__ mode = b.mode + q.p0;
  if (b.n_modes[g] < 0) {   // the pair kernel met a table entry outside [0, N): its matrix is NaN already
    for (int p = lane; p < P; p += 64) head[p] = mode[p] = -1;
    return;
  }
  const float* D = b.matrix + q.m0;
  const double cutoff = b.grp_cutoff[g];
  int nh = 0;
  for (int p = 0; p < P; ++p) {
    const float dpp = D[(size_t)p * P + p];
    if (dpp != dpp) {        // a coordinate that is not finite: never a head, compared with nobody
      if (lane == 0) head[p] = mode[p] = -1;
      continue;
    }
    int found = -1;
    for (int base = 0; base < nh && found < 0; base += 64) {
      const int h = base + lane;
      const bool ok = h < nh && (double)D[(size_t)heads[h] * P + p] <= cutoff;
      const unsigned long long m = __ballot(ok);
      if (m) found = base + __ffsll((long long)m) - 1;      // heads are kept in rank order: the lowest bit is the best-ranked head
    }
    if (found < 0) {
      if (lane == 0) heads[nh] = p;
      found = nh++;
      __syncthreads();
    }
    if (lane == 0) { head[p] = heads[found]; mode[p] = found; }
  }
  if (lane == 0) b.n_modes[g] = nh;
}

}  // namespace cbd

using namespace cbd;

int cbd_pose_modes(int32_t n_groups, int32_t max_n, int32_t max_p, int32_t n_poses, int32_t n_atoms, int32_t n_matrix, const int32_t* grp_n_dev,
                   const int32_t* grp_p_dev, const int32_t* grp_k_dev, const double* grp_cutoff_dev, const int32_t* pose_ptr_dev,
                   const int32_t* atom_ptr_dev, const int32_t* mat_ptr_dev, const float* pos_dev, const int32_t* const* idx_ref_tab_dev,
                   const int32_t* const* idx_pos_tab_dev, float* matrix_out_dev, int32_t* head_out_dev, int32_t* mode_out_dev,
                   int32_t* n_modes_out_dev, void* stream) {
  if (n_groups < 0 || max_n < 0 || max_p < 0 || n_poses < 0 || n_atoms < 0 || n_matrix < 0)
    return fail(CBD_ERR_ARG, "n_groups = %d, max_n = %d, max_p = %d, n_poses = %d, n_atoms = %d, n_matrix = %d", n_groups, max_n, max_p, n_poses,
                n_atoms, n_matrix);
  if (max_n > PC_MAX_N || max_p > PC_MAX_P)
    return fail(CBD_ERR_CAPACITY, "a ligand of %d atoms / a group of %d poses: the kernel takes up to %d / %d (cluster it on the host)", max_n, max_p,
                PC_MAX_N, PC_MAX_P);
  if (n_groups == 0) return 0;
  if (max_n < 1 || max_p < 1 || n_groups > 65535) return fail(CBD_ERR_ARG, "max_n = %d, max_p = %d with %d groups (at most 65535)", max_n, max_p, n_groups);
  if (!grp_n_dev || !grp_p_dev || !grp_k_dev || !grp_cutoff_dev || !pose_ptr_dev || !atom_ptr_dev || !mat_ptr_dev || !pos_dev || !idx_ref_tab_dev ||
      !idx_pos_tab_dev || !matrix_out_dev || !head_out_dev || !mode_out_dev || !n_modes_out_dev)
    return fail(CBD_ERR_ARG, "null argument");
  const size_t lds = (size_t)2 * max_n * PC_TILE * 3 * sizeof(float);
  if (lds > 48 * 1024) {   // the opt-in LDS size is a per-device function attribute
    static std::atomic<unsigned long long> attr_set{0};
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(attr_set.load(std::memory_order_acquire) & bit)) {
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pose_pair_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)((size_t)2 * PC_MAX_N * PC_TILE * 3 * sizeof(float))));
      attr_set.fetch_or(bit, std::memory_order_release);
    }
  }
  const PoseModesBatch b{n_groups, max_n, max_p, n_poses, n_atoms, n_matrix, grp_n_dev, grp_p_dev, grp_k_dev, grp_cutoff_dev, pose_ptr_dev,
                         atom_ptr_dev, mat_ptr_dev, pos_dev, idx_ref_tab_dev, idx_pos_tab_dev, matrix_out_dev, head_out_dev, mode_out_dev,
                         n_modes_out_dev};
  const int T = (max_p + PC_TILE - 1) / PC_TILE;
  hipLaunchKernelGGL(pose_pair_kernel, dim3(T * (T + 1) / 2, n_groups), dim3(64 * PC_WAVES), lds, reinterpret_cast<hipStream_t>(stream), b);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(pose_mode_kernel, dim3(n_groups), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), b);
  HIPCHK(hipGetLastError());
  return 0;
}
