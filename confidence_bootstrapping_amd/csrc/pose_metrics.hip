// What an inference epoch measures on its sampled poses, for P poses of C complexes in one launch (evaluation.pose_metrics_batch; per
// complex on the host: finetune_train.inference_epoch, evaluation.pose_metrics -- reference inference.py:505-548):
//     rmsd      = min over crystal poses q of float(sqrt(min_k S(q, k) / N)),  S(q, k) = sum_i |ref_q[idx_ref[k][i]] - pose[idx_pos[k][i]]|^2
//     centroid  = min over q of |mean(pose) - mean(ref_q)|
//     min_self  = the smallest distance between two different atoms of the pose
// One 256-thread workgroup per pose; the pose and the Q crystal poses of its complex live in LDS (fp32, as uploaded).  The ragged batch
// is described per COMPLEX (N, K, Q, where its crystal poses start, where its two [K][N] index tables are -- device pointers, because the
// tables of a ligand stay resident between calls and are not part of the upload) and per POSE (its complex, where its atoms start).
// S(q, k) is symm_rmsd_kernel's (kernels.hip) to the bit: one wave per (q, k), lane l adds atoms l, l + 64, ... in fp64 with the same
// expression, then wave_sum_d.  The K mappings are dealt over the four waves (wave w takes k = w, w + 4, ...); each wave keeps its first
// minimum, lane 0 parks it in LDS, and every thread folds the four by (smaller S, then smaller k) -- the serial kernel's "first minimum
// wins" whichever wave found it.  Across crystal poses the fp32 RMSDs are compared, lowest q first, as the host's np.min / np.argmin over
// the per-crystal-pose results does.  centroid and min_self are fp64 on the fp32 coordinates and round to fp32 once.
// No atomics, no global scratch; every sum has a fixed order, so a pose's result depends neither on the run nor on what shares the launch.
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "host_util.h"
#include "pose_math.h"

namespace cbd {

constexpr int PM_MAX_N = 512;          // atoms of a ligand
constexpr int PM_MAX_REF = 4096;       // Q * N atoms of a complex's crystal poses; (512 + 4096) * 12 B = 54 KB of LDS at the limit
constexpr int PM_WAVES = 4;

struct PoseMetricsBatch {
  int P, C, max_n, max_ref;
  const int* pose_cplx;            // [P] complex of the pose
  const int* pose_ptr;             // [P + 1] atoms of pos
  const float* pos;                // [sum N over P][3]
  const int* cplx_n;               // [C]
  const int* cplx_k;               // [C]
  const int* cplx_q;               // [C]
  const int* ref_ptr;              // [C + 1] atoms of ref (Q * N per complex)
  const float* ref;                // [sum Q N over C][3]
  const int* const* idx_ref;       // [C] -> [K][N]
  const int* const* idx_pos;       // [C] -> [K][N]
  float* rmsd;                     // [P]
  float* centroid;                 // [P]
  float* min_self;                 // [P]
  int* argmin_ref;                 // [P]
  int* argmin_iso;                 // [P]
};

CBD_DEV double wave_min_d(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
  return v;
}

// grid: P workgroups of four waves; dynamic LDS: (max_n + max_ref) * 3 floats
__global__ __launch_bounds__(256) void pose_metrics_kernel(PoseMetricsBatch b) {
  extern __shared__ float coords[];   // pose [max_n][3], then the complex's crystal poses [Q][N][3]
  __shared__ double w_s[PM_WAVES];
  __shared__ int w_k[PM_WAVES];
  const int p = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  // the description of the pose, checked before anything is indexed with it (workgroup-uniform)
  const int c = b.pose_cplx[p];
  bool good = c >= 0 && c < b.C;
  int N = 0, K = 0, Q = 0, a0 = 0, r0 = 0;
  const int* __restrict__ IR = nullptr;
  const int* __restrict__ IP = nullptr;
  if (good) {
    N = b.cplx_n[c]; K = b.cplx_k[c]; Q = b.cplx_q[c];
    a0 = b.pose_ptr[p]; r0 = b.ref_ptr[c];
    IR = b.idx_ref[c]; IP = b.idx_pos[c];
    good = N >= 1 && N <= b.max_n && K >= 1 && Q >= 1 && (long long)Q * N <= (long long)b.max_ref && a0 >= 0 && b.pose_ptr[p + 1] - a0 == N &&
           r0 >= 0 && (long long)(b.ref_ptr[c + 1] - r0) == (long long)Q * N && IR != nullptr && IP != nullptr;
  }
  if (!good) {   // a complex that does not exist, sizes that contradict each other or the launch, no index table: NaN, nothing indexed
    if (tid == 0) {
      b.rmsd[p] = b.centroid[p] = b.min_self[p] = __builtin_nanf("");
      b.argmin_ref[p] = b.argmin_iso[p] = -1;
    }
    return;
  }
  float* __restrict__ pose = coords;
  float* __restrict__ refs = coords + (size_t)b.max_n * 3;
  {
    const float* __restrict__ gp = b.pos + (size_t)a0 * 3;
    const float* __restrict__ gr = b.ref + (size_t)r0 * 3;
    for (int i = tid; i < 3 * N; i += 256) pose[i] = gp[i];
    for (int i = tid; i < 3 * Q * N; i += 256) refs[i] = gr[i];
  }
  __syncthreads();

  // ---- symmetry-corrected RMSD
  bool in = true;              // every index this thread read named an atom
  float best_r = 0.f;
  int best_q = 0, best_k = 0;
  for (int q = 0; q < Q; ++q) {
    const float* __restrict__ ref = refs + (size_t)q * N * 3;
    double wbest = 1.0e300;
    int wk = 0x7fffffff;
    for (int k = wave; k < K; k += PM_WAVES) {
      double s = 0.0;
      for (int i = lane; i < N; i += 64) {
        int ir = IR[(size_t)k * N + i], ip = IP[(size_t)k * N + i];
        if ((unsigned)ir >= (unsigned)N || (unsigned)ip >= (unsigned)N) { in = false; ir = 0; ip = 0; }   // reported below; LDS is not indexed with it
        const double dx = (double)ref[3 * ir] - (double)pose[3 * ip], dy = (double)ref[3 * ir + 1] - (double)pose[3 * ip + 1],
                     dz = (double)ref[3 * ir + 2] - (double)pose[3 * ip + 2];
        s += dx * dx + dy * dy + dz * dz;
      }
      s = wave_sum_d(s);
      if (s < wbest) { wbest = s; wk = k; }
    }
    if (lane == 0) { w_s[wave] = wbest; w_k[wave] = wk; }
    __syncthreads();
    double best = 1.0e300;
    int bk = 0;
    for (int w = 0; w < PM_WAVES; ++w) {
      const double sw = w_s[w];
      const int kw = w_k[w];
      if (sw < best || (sw == best && kw < bk)) { best = sw; bk = kw; }
    }
    const float r = (float)sqrt(best / (double)N);
    if (q == 0 || r < best_r) { best_r = r; best_q = q; best_k = bk; }
    __syncthreads();   // w_s / w_k are written again for the next crystal pose
  }
  const bool bad = __syncthreads_or(in ? 0 : 1) != 0;

  // ---- centroid distance (every wave computes the same values; only thread 0 writes them)
  double pc[3], rc[3];
  wave_centroid_d(pose, N, lane, pc);
  float best_c = 0.f;
  for (int q = 0; q < Q; ++q) {
    wave_centroid_d(refs + (size_t)q * N * 3, N, lane, rc);
    const double dx = pc[0] - rc[0], dy = pc[1] - rc[1], dz = pc[2] - rc[2];
    const float d = (float)sqrt(dx * dx + dy * dy + dz * dz);
    if (q == 0 || d < best_c) best_c = d;
  }

  // ---- smallest distance between two different atoms: thread t takes atoms t, t + 256 against all others (an LDS broadcast per j)
  double m2 = __builtin_inf();
  for (int i = tid; i < N; i += 256) {
    const double xi = pose[3 * i], yi = pose[3 * i + 1], zi = pose[3 * i + 2];
    for (int j = 0; j < N; ++j) {
      if (j == i) continue;
      const double dx = xi - (double)pose[3 * j], dy = yi - (double)pose[3 * j + 1], dz = zi - (double)pose[3 * j + 2];
      m2 = fmin(m2, dx * dx + dy * dy + dz * dz);
    }
  }
  m2 = wave_min_d(m2);
  if (lane == 0) w_s[wave] = m2;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < PM_WAVES; ++w) m2 = fmin(m2, w_s[w]);
    if (bad) {   // an isomorphism that names no atom: NaN for this pose
      b.rmsd[p] = b.centroid[p] = b.min_self[p] = __builtin_nanf("");
      b.argmin_ref[p] = b.argmin_iso[p] = -1;
    } else {
      b.rmsd[p] = best_r;
      b.centroid[p] = best_c;
      b.min_self[p] = (float)sqrt(m2);   // a single atom has no pair: inf, like the host's masked cdist
      b.argmin_ref[p] = best_q;
      b.argmin_iso[p] = best_k;
    }
  }
}

}  // namespace cbd

using namespace cbd;

int cbd_pose_metrics(int32_t n_poses, int32_t n_complexes, int32_t max_n, int32_t max_ref_atoms, const int32_t* pose_cplx_dev,
                     const int32_t* pose_ptr_dev, const float* pos_dev, const int32_t* cplx_n_dev, const int32_t* cplx_k_dev,
                     const int32_t* cplx_q_dev, const int32_t* ref_ptr_dev, const float* ref_dev, const int32_t* const* idx_ref_tab_dev,
                     const int32_t* const* idx_pos_tab_dev, float* rmsd_out_dev, float* centroid_out_dev, float* min_self_out_dev,
                     int32_t* argmin_ref_out_dev, int32_t* argmin_iso_out_dev, void* stream) {
  if (n_poses < 0 || n_complexes < 0 || max_n < 0 || max_ref_atoms < 0)
    return fail(CBD_ERR_ARG, "n_poses = %d, n_complexes = %d, max_n = %d, max_ref_atoms = %d", n_poses, n_complexes, max_n, max_ref_atoms);
  if (max_n > PM_MAX_N || max_ref_atoms > PM_MAX_REF)
    return fail(CBD_ERR_CAPACITY, "a ligand of %d atoms / %d crystal-pose atoms: the kernel takes up to %d / %d (measure it on the host)", max_n,
                max_ref_atoms, PM_MAX_N, PM_MAX_REF);
  if (n_poses == 0) return 0;
  if (max_n < 1 || max_ref_atoms < max_n || n_complexes < 1)
    return fail(CBD_ERR_ARG, "max_n = %d, max_ref_atoms = %d, n_complexes = %d with %d poses", max_n, max_ref_atoms, n_complexes, n_poses);
  if (!pose_cplx_dev || !pose_ptr_dev || !pos_dev || !cplx_n_dev || !cplx_k_dev || !cplx_q_dev || !ref_ptr_dev || !ref_dev || !idx_ref_tab_dev ||
      !idx_pos_tab_dev || !rmsd_out_dev || !centroid_out_dev || !min_self_out_dev || !argmin_ref_out_dev || !argmin_iso_out_dev)
    return fail(CBD_ERR_ARG, "null argument");
  const PoseMetricsBatch b{n_poses, n_complexes, max_n, max_ref_atoms, pose_cplx_dev, pose_ptr_dev, pos_dev, cplx_n_dev, cplx_k_dev, cplx_q_dev,
                           ref_ptr_dev, ref_dev, idx_ref_tab_dev, idx_pos_tab_dev, rmsd_out_dev, centroid_out_dev, min_self_out_dev,
                           argmin_ref_out_dev, argmin_iso_out_dev};
  const size_t lds = ((size_t)max_n + (size_t)max_ref_atoms) * 3 * sizeof(float);
  hipLaunchKernelGGL(pose_metrics_kernel, dim3(n_poses), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), b);
  HIPCHK(hipGetLastError());
  return 0;
}
