// Starting poses of an inference epoch in one launch: what randomize_position (sampling.py; reference utils/sampling.py:15-48) does to
// every copy of every complex, for P poses of C complexes at once.  The random draws stay on the host (sampling.draw_randomization);
// this kernel only moves the atoms:
//     flex = pos_in;  for bond r = 0 .. R-1 in edge_mask order, skipped when tor[r] == 0 (utils/torsion.py:48-72, NO Kabsch afterwards):
//         axis = flex[u] - flex[v];  the atoms of mask_rotate[r] turn by tor[r] about that axis through flex[v]
//     c = mean(flex);  out = (flex - c) Rm^T + center[complex of the pose] (+ tr)        Rm is GIVEN (scipy's matrix cast to fp32)
// One wavefront per pose, atoms strided over its lanes, the pose in LDS.  The ragged description is that of noise_transform.hip
// (lig_ptr / rot_ptr / mask_ptr prefix sums, mask_rotate packed one bit per atom, ceil(Nl / 32) words per bond) behind one level of
// indirection: pose_lig[p] names one of L ligand descriptions (start coordinates, bonds, masks), so the 40 copies of a complex share one.
// Precision: the pose lives in LDS as fp32 like the host's array; a bond's rotation matrix (wave-uniform, one per bond) and its product
// with the atoms are fp64 and round to fp32 once per bond -- what the host path does with scipy / numpy, and what its deviation from
// fp64, the yardstick of tests/test_gpu_randomize_batch.py, is made of.  The fp32 quaternion route of pose_math.h was NOT tried against
// that bound: fp64 was chosen up front, on the estimate that fp32 matrix entries (a few 1e-7 relative) times the lever of a far atom
// come close to it; at one matrix per bond the cost is nothing.  The centroid (wave_centroid_d) and the last move are fp64 as well and round once.
// No atomics; every sum has a fixed order, so a pose's result depends neither on the run nor on what shares the launch.
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "host_util.h"
#include "pose_math.h"

namespace cbd {

constexpr int RP_MAX_NL = 512;    // 512 x 3 floats of LDS per wave
constexpr int RP_MAX_R = 128;

struct RandomizeBatch {
  int P, L, C, max_nl, max_r;
  const int* pose_lig;            // [P] ligand description of the pose
  const int* pose_cplx;           // [P] complex of the pose (row of center)
  const int* out_ptr;             // [P + 1] atoms of pos_out
  const int* tor_ptr;             // [P + 1] entries of tor
  const int* lig_ptr;             // [L + 1] atoms
  const int* rot_ptr;             // [L + 1] rotatable bonds
  const int* mask_ptr;            // [L + 1] words of mask_bits
  const float* pos_in;            // [sum Nl over L][3]
  const int* rot_edge;            // [sum R over L][2]  local (u, v), edge_mask order
  const unsigned* mask_bits;      // per ligand [R][ceil(Nl / 32)]
  const double* tor;              // [sum R over P] or null (no_torsion); fp64, as the host draws them
  const float* rot_mat;           // [P][9] row-major
  const float* tr;                // [P][3] or null (no_random)
  const float* center;            // [C][3]
  float* pos_out;                 // [sum Nl over P][3]
};

// rotation by `th` about the unit vector (kx, ky, kz): Rodrigues, I + sin K + (1 - cos) K^2
CBD_DEV void axis_turn_d(double kx, double ky, double kz, double th, double (&Q)[9]) {
  const double s = sin(th), c1 = 1.0 - cos(th);
  Q[0] = 1.0 - c1 * (ky * ky + kz * kz); Q[1] = c1 * kx * ky - s * kz;          Q[2] = c1 * kx * kz + s * ky;
  Q[3] = c1 * kx * ky + s * kz;          Q[4] = 1.0 - c1 * (kx * kx + kz * kz); Q[5] = c1 * ky * kz - s * kx;
  Q[6] = c1 * kx * kz - s * ky;          Q[7] = c1 * ky * kz + s * kx;          Q[8] = 1.0 - c1 * (kx * kx + ky * ky);
}

// grid: P workgroups of one wave; dynamic LDS: max_nl * 3 floats
__global__ __launch_bounds__(64) void randomize_poses_kernel(RandomizeBatch rb) {
  extern __shared__ float flex[];   // [Nl][3]
  const int p = blockIdx.x, lane = lane_id();
  const int o0 = rb.out_ptr[p], No = rb.out_ptr[p + 1] - o0;
  // a pose outside the sizes the launch declared (the host sized the LDS and checked the capacity with them) is not touched
  if (o0 < 0 || No < 1 || No > rb.max_nl) return;
  float* __restrict__ O = rb.pos_out + (size_t)o0 * 3;
  const int l = rb.pose_lig[p], cx = rb.pose_cplx[p];
  bool good = l >= 0 && l < rb.L && cx >= 0 && cx < rb.C;
  int a0 = 0, Nl = 0, r0 = 0, R = 0, t0 = 0;
  const bool with_tor = rb.tor != nullptr && rb.max_r > 0;
  if (good) {
    a0 = rb.lig_ptr[l]; Nl = rb.lig_ptr[l + 1] - a0;
    good = a0 >= 0 && Nl == No;
    if (with_tor) {
      r0 = rb.rot_ptr[l]; R = rb.rot_ptr[l + 1] - r0;
      t0 = rb.tor_ptr[p];
      if (R > rb.max_r) return;
      good = good && R >= 0 && r0 >= 0 && t0 >= 0 && rb.tor_ptr[p + 1] - t0 == R && rb.mask_ptr[l] >= 0;
    }
  }
  const bool flexible = with_tor && R > 0;
  const int* __restrict__ E = flexible ? rb.rot_edge + (size_t)r0 * 2 : nullptr;
  if (good && flexible) good = bond_ends_are_atoms(E, R, Nl, lane);   // the torsion loop indexes LDS with them
  if (!good) {   // an index that names no ligand / complex, sizes that contradict each other, a bond end that is no atom: NaN, nothing indexed with it
    for (int i = lane; i < 3 * No; i += 64) O[i] = __builtin_nanf("");
    return;
  }
  const float* __restrict__ P = rb.pos_in + (size_t)a0 * 3;
  for (int i = lane; i < 3 * Nl; i += 64) flex[i] = P[i];
  __syncthreads();
  if (flexible) {
    const int words = (Nl + 31) >> 5;
    const unsigned* __restrict__ M = rb.mask_bits + rb.mask_ptr[l];
    const double* __restrict__ tor = rb.tor + t0;
    // sequential torsions on the already-updated coordinates
    for (int rho = 0; rho < R; ++rho) {
      const double th = tor[rho];
      if (th == 0.0) continue;   // utils/torsion.py:55 (wave-uniform)
      const int u = E[2 * rho], v = E[2 * rho + 1];
      const double vx = flex[3 * v], vy = flex[3 * v + 1], vz = flex[3 * v + 2];
      const double ax = (double)flex[3 * u] - vx, ay = (double)flex[3 * u + 1] - vy, az = (double)flex[3 * u + 2] - vz;
      const double n = sqrt(ax * ax + ay * ay + az * az);
      double Q[9];
      axis_turn_d(ax / n, ay / n, az / n, th, Q);
      __syncthreads();
      const unsigned* __restrict__ row = M + (size_t)rho * words;
      for (int a = lane; a < Nl; a += 64) {
        if (mask_bit(row, a)) {
          const double x = (double)flex[3 * a] - vx, y = (double)flex[3 * a + 1] - vy, z = (double)flex[3 * a + 2] - vz;
          flex[3 * a] = (float)(Q[0] * x + Q[1] * y + Q[2] * z + vx);
          flex[3 * a + 1] = (float)(Q[3] * x + Q[4] * y + Q[5] * z + vy);
          flex[3 * a + 2] = (float)(Q[6] * x + Q[7] * y + Q[8] * z + vz);
        }
      }
      __syncthreads();
    }
  }
  double c[3];
  wave_centroid_d(flex, Nl, lane, c);
  double Rm[9], t[3];
  for (int k = 0; k < 9; ++k) Rm[k] = (double)rb.rot_mat[(size_t)p * 9 + k];
  for (int k = 0; k < 3; ++k) t[k] = (double)rb.center[(size_t)cx * 3 + k] + (rb.tr ? (double)rb.tr[(size_t)p * 3 + k] : 0.0);
  for (int a = lane; a < Nl; a += 64) {
    const double x = flex[3 * a] - c[0], y = flex[3 * a + 1] - c[1], z = flex[3 * a + 2] - c[2];
    O[3 * a] = (float)(Rm[0] * x + Rm[1] * y + Rm[2] * z + t[0]);
    O[3 * a + 1] = (float)(Rm[3] * x + Rm[4] * y + Rm[5] * z + t[1]);
    O[3 * a + 2] = (float)(Rm[6] * x + Rm[7] * y + Rm[8] * z + t[2]);
  }
}

}  // namespace cbd

using namespace cbd;

int cbd_randomize_poses(int32_t n_poses, int32_t n_ligands, int32_t n_complexes, int32_t max_nl, int32_t max_r,
                        const int32_t* pose_lig_dev, const int32_t* pose_cplx_dev, const int32_t* out_ptr_dev, const int32_t* tor_ptr_dev,
                        const int32_t* lig_ptr_dev, const float* pos_in_dev, const int32_t* rot_ptr_dev, const int32_t* rot_edge_dev,
                        const int32_t* mask_ptr_dev, const uint32_t* mask_bits_dev, const double* tor_dev, const float* rot_mat_dev,
                        const float* tr_dev, const float* center_dev, float* pos_out_dev, void* stream) {
  if (n_poses < 0 || n_ligands < 0 || n_complexes < 0 || max_nl < 0 || max_r < 0)
    return fail(CBD_ERR_ARG, "n_poses = %d, n_ligands = %d, n_complexes = %d, max_nl = %d, max_r = %d", n_poses, n_ligands, n_complexes, max_nl, max_r);
  if (max_nl > RP_MAX_NL || max_r > RP_MAX_R)
    return fail(CBD_ERR_CAPACITY, "a ligand of %d atoms / %d rotatable bonds: the kernel takes up to %d / %d (move it on the host)", max_nl,
                max_r, RP_MAX_NL, RP_MAX_R);
  if (n_poses == 0) return 0;
  if (max_nl < 1 || n_ligands < 1 || n_complexes < 1)
    return fail(CBD_ERR_ARG, "max_nl = %d, n_ligands = %d, n_complexes = %d with %d poses", max_nl, n_ligands, n_complexes, n_poses);
  if (!pose_lig_dev || !pose_cplx_dev || !out_ptr_dev || !lig_ptr_dev || !pos_in_dev || !rot_mat_dev || !center_dev || !pos_out_dev)
    return fail(CBD_ERR_ARG, "null argument");
  if (tor_dev && max_r > 0 && (!tor_ptr_dev || !rot_ptr_dev || !rot_edge_dev || !mask_ptr_dev || !mask_bits_dev))
    return fail(CBD_ERR_ARG, "torsion updates without bonds / masks");
  const RandomizeBatch rb{n_poses, n_ligands, n_complexes, max_nl, max_r, pose_lig_dev, pose_cplx_dev, out_ptr_dev, tor_ptr_dev,
                          lig_ptr_dev, rot_ptr_dev, mask_ptr_dev, pos_in_dev, rot_edge_dev, mask_bits_dev, tor_dev, rot_mat_dev,
                          tr_dev, center_dev, pos_out_dev};
  hipLaunchKernelGGL(randomize_poses_kernel, dim3(n_poses), dim3(64), (size_t)max_nl * 3 * sizeof(float), reinterpret_cast<hipStream_t>(stream), rb);
  HIPCHK(hipGetLastError());
  return 0;
}
