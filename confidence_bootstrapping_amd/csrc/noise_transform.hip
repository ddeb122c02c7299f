// Forward-diffusion move of a whole fine-tuning batch in one launch: what NoiseTransform.apply_noise does to the pose of every buffered
// item (reference datasets/pdbbind.py:60-110 -> utils/diffusion_utils.py:33-58 `modify_conformer`, pivot = None), for P DIFFERENT
// ligands at once -- each with its own atom count Nl, rotatable bonds R and mask_rotate.  The random draws stay on the host
// (NoiseTransform.draw); this kernel only moves the atoms:
//     c = centroid(pos);  rigid = (pos - c) Rm^T + tr + c  with Rm = axis_angle_to_matrix(rot)   (quaternion route, utils/geometry.py:39-86)
//     flex = rigid;  for bond r = 0 .. R-1 in order, skipped when tor[r] == 0 (utils/torsion.py:48-72):
//         axis = flex[u] - flex[v];  the atoms of mask_rotate[r] turn by tor[r] about that axis through flex[v]
//     out = flex moved rigidly onto `rigid` in the least-squares sense (Kabsch, utils/geometry.py:209-243);  R = 0 or no torsion: out = rigid
// One wavefront per ligand, atoms strided over its lanes, both poses in LDS; the arithmetic is pose_update_kernel's (kernels.hip), with
// the helpers of pose_math.h: the quaternion route for the rotations and horn_rotation for the alignment.  This kernel's own: the
// centroids of the alignment, S and the last move are fp64.  The ragged description is CSR-like:
// lig_ptr / rot_ptr / mask_ptr are prefix sums over the ligands; mask_rotate is packed one bit per atom, ceil(Nl / 32) words per bond.
// No atomics; every sum has a fixed order, so a ligand's result does not depend on the run nor on what shares the launch.
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "host_util.h"
#include "pose_math.h"

namespace cbd {

constexpr int NT_MAX_NL = 512;    // 2 x 512 x 3 floats of LDS per wave
constexpr int NT_MAX_R = 128;

struct NoiseBatch {
  int P, max_nl, max_r;
  const int* lig_ptr;             // [P + 1] atoms
  const int* rot_ptr;             // [P + 1] rotatable bonds
  const int* mask_ptr;            // [P + 1] words of mask_bits
  const float* pos_in;            // [sum Nl][3]
  const int* rot_edge;            // [sum R][2]  local (u, v), edge_mask order
  const unsigned* mask_bits;      // per ligand [R][ceil(Nl / 32)]
  const float* tr;                // [P][3]
  const float* rot;               // [P][3]
  const float* tor;               // [sum R] or null (no_torsion)
  float* pos_out;                 // [sum Nl][3]
};

// grid: P workgroups of one wave; dynamic LDS: max_nl * 6 floats
__global__ __launch_bounds__(64) void noise_conformers_kernel(NoiseBatch nb) {
  extern __shared__ float sp[];   // [Nl][3] flexible pose, [Nl][3] rigid pose
  const int p = blockIdx.x, lane = lane_id();
  const int a0 = nb.lig_ptr[p], Nl = nb.lig_ptr[p + 1] - a0;
  const int r0 = nb.rot_ptr[p], R = nb.rot_ptr[p + 1] - r0;
  const int words = (Nl + 31) >> 5;
  // a ligand outside the sizes the launch declared (the host sized the LDS and checked the capacity with them) is not touched
  if (Nl < 1 || Nl > nb.max_nl || R < 0 || R > nb.max_r || a0 < 0 || r0 < 0) return;
  const float* __restrict__ P = nb.pos_in + (size_t)a0 * 3;
  float* __restrict__ O = nb.pos_out + (size_t)a0 * 3;
  const float* __restrict__ tor = nb.tor ? nb.tor + r0 : nullptr;
  const int* __restrict__ E = nb.rot_edge + (size_t)r0 * 2;
  const bool flexible = tor != nullptr && R > 0;
  const unsigned* __restrict__ M = flexible ? nb.mask_bits + nb.mask_ptr[p] : nullptr;
  if (flexible && !bond_ends_are_atoms(E, R, Nl, lane)) {   // the torsion loop indexes LDS with them
    for (int i = lane; i < 3 * Nl; i += 64) O[i] = __builtin_nanf("");
    return;
  }
  float* flex = sp;
  float* rigid = sp + 3 * Nl;
  const float trp[3] = {nb.tr[p * 3], nb.tr[p * 3 + 1], nb.tr[p * 3 + 2]};
  // centroid
  float cx = 0.f, cy = 0.f, cz = 0.f;
  for (int a = lane; a < Nl; a += 64) { cx += P[3 * a]; cy += P[3 * a + 1]; cz += P[3 * a + 2]; }
  cx = wave_sum(cx) / (float)Nl; cy = wave_sum(cy) / (float)Nl; cz = wave_sum(cz) / (float)Nl;
  float Rm[9];
  axis_angle_to_matrix(nb.rot[p * 3], nb.rot[p * 3 + 1], nb.rot[p * 3 + 2], Rm);
  for (int a = lane; a < Nl; a += 64) {
    const float x = P[3 * a] - cx, y = P[3 * a + 1] - cy, z = P[3 * a + 2] - cz;
    const float nx = Rm[0] * x + Rm[1] * y + Rm[2] * z + trp[0] + cx;
    const float ny = Rm[3] * x + Rm[4] * y + Rm[5] * z + trp[1] + cy;
    const float nz = Rm[6] * x + Rm[7] * y + Rm[8] * z + trp[2] + cz;
    if (flexible) {
      rigid[3 * a] = nx; rigid[3 * a + 1] = ny; rigid[3 * a + 2] = nz;
      flex[3 * a] = nx; flex[3 * a + 1] = ny; flex[3 * a + 2] = nz;
    } else {
      O[3 * a] = nx; O[3 * a + 1] = ny; O[3 * a + 2] = nz;
    }
  }
  if (!flexible) return;
  __syncthreads();
  // sequential torsions on the already-updated coordinates
  for (int rho = 0; rho < R; ++rho) {
    const float th = tor[rho];
    if (th == 0.f) continue;   // utils/torsion.py:55 (wave-uniform)
    const int u = E[2 * rho], v = E[2 * rho + 1];
    const float vx = flex[3 * v], vy = flex[3 * v + 1], vz = flex[3 * v + 2];
    float ax = flex[3 * u] - vx, ay = flex[3 * u + 1] - vy, az = flex[3 * u + 2] - vz;
    const float n = sqrtf(ax * ax + ay * ay + az * az);
    ax = ax / n * th; ay = ay / n * th; az = az / n * th;
    float Q[9];
    axis_angle_to_matrix(ax, ay, az, Q);
    __syncthreads();
    const unsigned* __restrict__ row = M + (size_t)rho * words;
    for (int a = lane; a < Nl; a += 64) {
      if (mask_bit(row, a)) {
        const float x = flex[3 * a] - vx, y = flex[3 * a + 1] - vy, z = flex[3 * a + 2] - vz;
        flex[3 * a] = Q[0] * x + Q[1] * y + Q[2] * z + vx;
        flex[3 * a + 1] = Q[3] * x + Q[4] * y + Q[5] * z + vy;
        flex[3 * a + 2] = Q[6] * x + Q[7] * y + Q[8] * z + vz;
      }
    }
    __syncthreads();
  }
  // Kabsch: R, t minimising |R flex + t - rigid|  (the steps of pose_update_kernel; the two centroids and the final move are kept in
  // fp64 here -- a fp32 sum over up to 512 coordinates of tens of A would cost the output centroid more than the host path loses)
  double fa[3], fb[3];
  wave_centroid_d(flex, Nl, lane, fa);
  wave_centroid_d(rigid, Nl, lane, fb);
  double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int a = lane; a < Nl; a += 64) {
    const double am[3] = {flex[3 * a] - fa[0], flex[3 * a + 1] - fa[1], flex[3 * a + 2] - fa[2]};
    const double bm[3] = {rigid[3 * a] - fb[0], rigid[3 * a + 1] - fb[1], rigid[3 * a + 2] - fb[2]};
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) S[3 * i + k] += am[i] * bm[k];
  }
  for (int i = 0; i < 9; ++i) S[i] = wave_sum_d(S[i]);
  double Rk[9];
  horn_rotation(S, Rk);
  // aligned = R (flex - ca) + cb
  for (int a = lane; a < Nl; a += 64) {
    const double fx = flex[3 * a] - fa[0], fy = flex[3 * a + 1] - fa[1], fz = flex[3 * a + 2] - fa[2];
    O[3 * a] = (float)(Rk[0] * fx + Rk[1] * fy + Rk[2] * fz + fb[0]);
    O[3 * a + 1] = (float)(Rk[3] * fx + Rk[4] * fy + Rk[5] * fz + fb[1]);
    O[3 * a + 2] = (float)(Rk[6] * fx + Rk[7] * fy + Rk[8] * fz + fb[2]);
  }
}

}  // namespace cbd

using namespace cbd;

int cbd_noise_conformers(int32_t n_ligands, int32_t max_nl, int32_t max_r, const int32_t* lig_ptr_dev, const float* pos_in_dev,
                         const int32_t* rot_ptr_dev, const int32_t* rot_edge_dev, const int32_t* mask_ptr_dev, const uint32_t* mask_bits_dev,
                         const float* tr_dev, const float* rot_dev, const float* tor_dev, float* pos_out_dev, void* stream) {
  if (n_ligands < 0 || max_nl < 0 || max_r < 0) return fail(CBD_ERR_ARG, "n_ligands = %d, max_nl = %d, max_r = %d", n_ligands, max_nl, max_r);
  if (max_nl > NT_MAX_NL || max_r > NT_MAX_R)
    return fail(CBD_ERR_CAPACITY, "a ligand of %d atoms / %d rotatable bonds: the kernel takes up to %d / %d (move it on the host)", max_nl,
                max_r, NT_MAX_NL, NT_MAX_R);
  if (n_ligands == 0) return 0;
  if (max_nl < 1) return fail(CBD_ERR_ARG, "max_nl = %d with %d ligands", max_nl, n_ligands);
  if (!lig_ptr_dev || !pos_in_dev || !rot_ptr_dev || !mask_ptr_dev || !tr_dev || !rot_dev || !pos_out_dev)
    return fail(CBD_ERR_ARG, "null argument");
  if (tor_dev && max_r > 0 && (!rot_edge_dev || !mask_bits_dev)) return fail(CBD_ERR_ARG, "torsion updates without bonds / masks");
  const NoiseBatch nb{n_ligands, max_nl, max_r, lig_ptr_dev, rot_ptr_dev, mask_ptr_dev, pos_in_dev, rot_edge_dev, mask_bits_dev,
                      tr_dev, rot_dev, tor_dev, pos_out_dev};
  hipLaunchKernelGGL(noise_conformers_kernel, dim3(n_ligands), dim3(64), (size_t)max_nl * 6 * sizeof(float), reinterpret_cast<hipStream_t>(stream), nb);
  HIPCHK(hipGetLastError());
  return 0;
}
