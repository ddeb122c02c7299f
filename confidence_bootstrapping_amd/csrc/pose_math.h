// Device helpers of the pose arithmetic, the one home of what the pose kernels share (pose_update_kernel in kernels.hip,
// noise_transform.hip, randomize_poses.hip, pose_metrics.hip, torsion_match.hip): the fp32 quaternion route from an axis-angle vector
// to its rotation matrix, the 64-lane butterfly sums and the fp64 centroid, Horn's least-squares alignment by fp64 Jacobi, and the
// checks of the ragged ligand description.  What differs between the kernels on purpose stays with them: how S is accumulated, the
// precision of the centroids and of the final move, and the sequential-torsion loops (mask format, precision, skip rule and where the
// atoms live all differ).
#pragma once
#include <hip/hip_runtime.h>

#include "device_util.h"

namespace cbd {

CBD_DEV void axis_angle_to_matrix(float ax, float ay, float az, float (&R)[9]) {
  // via quaternion, incl. the |angle| < 1e-6 series branch (utils/geometry.py:39-86)
  const float ang = sqrtf(ax * ax + ay * ay + az * az);
  const float half = 0.5f * ang;
  const float k = fabsf(ang) < 1e-6f ? 0.5f - (ang * ang) / 48.f : sinf(half) / ang;
  const float r = cosf(half), i = ax * k, j = ay * k, kk = az * k;
  const float two_s = 2.0f / (r * r + i * i + j * j + kk * kk);
  R[0] = 1 - two_s * (j * j + kk * kk); R[1] = two_s * (i * j - kk * r);     R[2] = two_s * (i * kk + j * r);
  R[3] = two_s * (i * j + kk * r);     R[4] = 1 - two_s * (i * i + kk * kk); R[5] = two_s * (j * kk - i * r);
  R[6] = two_s * (i * kk - j * r);     R[7] = two_s * (j * kk + i * r);     R[8] = 1 - two_s * (i * i + j * j);
}

CBD_DEV float wave_sum(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
CBD_DEV double wave_sum_d(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// centroid of n atoms in LDS, the same value in every lane
CBD_DEV void wave_centroid_d(const float* __restrict__ x, int n, int lane, double (&c)[3]) {
  c[0] = c[1] = c[2] = 0.0;
  for (int a = lane; a < n; a += 64)
    for (int k = 0; k < 3; ++k) c[k] += (double)x[3 * a + k];
  for (int k = 0; k < 3; ++k) c[k] = wave_sum_d(c[k]) / (double)n;
}

// Horn's symmetric 4x4 matrix of S = sum a b^T: its largest eigenvalue's eigenvector is the quaternion of the rotation that takes a onto b
CBD_DEV void horn_matrix(const double (&S)[9], double (&N)[4][4]) {
  N[0][0] = S[0] + S[4] + S[8]; N[0][1] = S[5] - S[7];        N[0][2] = S[6] - S[2];         N[0][3] = S[1] - S[3];
  N[1][0] = S[5] - S[7];        N[1][1] = S[0] - S[4] - S[8]; N[1][2] = S[1] + S[3];         N[1][3] = S[6] + S[2];
  N[2][0] = S[6] - S[2];        N[2][1] = S[1] + S[3];        N[2][2] = -S[0] + S[4] - S[8]; N[2][3] = S[5] + S[7];
  N[3][0] = S[1] - S[3];        N[3][1] = S[6] + S[2];        N[3][2] = S[5] + S[7];         N[3][3] = -S[0] - S[4] + S[8];
}

// 12 sweeps of cyclic Jacobi on a symmetric 4x4 matrix in fp64: N becomes diagonal (the eigenvalues).  WITH_VECTORS: V (the identity
// on entry) collects the rotations, its columns become the eigenvectors; otherwise V is not touched.  EARLY_EXIT: stop once the
// off-diagonal part is below fp64 resolution of the diagonal.
template <bool WITH_VECTORS, bool EARLY_EXIT>
CBD_DEV void jacobi_sweeps(double (&N)[4][4], double (*V)[4]) {
  for (int sweep = 0; sweep < 12; ++sweep) {
    if (EARLY_EXIT) {
      const double off = fabs(N[0][1]) + fabs(N[0][2]) + fabs(N[0][3]) + fabs(N[1][2]) + fabs(N[1][3]) + fabs(N[2][3]);
      const double dia = fabs(N[0][0]) + fabs(N[1][1]) + fabs(N[2][2]) + fabs(N[3][3]);
      if (off <= 1e-18 * dia) break;
    }
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = N[p][q];
        if (fabs(apq) < 1e-280) continue;
        const double th = (N[q][q] - N[p][p]) / (2.0 * apq);
        const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // N <- N J
          const double nkp = N[k][p], nkq = N[k][q];
          N[k][p] = c * nkp - s * nkq; N[k][q] = s * nkp + c * nkq;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // N <- J^T N
          const double npk = N[p][k], nqk = N[q][k];
          N[p][k] = c * npk - s * nqk; N[q][k] = s * npk + c * nqk;
        }
        if (WITH_VECTORS) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double vkp = V[k][p], vkq = V[k][q];
            V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
          }
        }
      }
  }
}

// the proper rotation R (row-major) minimising sum |R a - b|^2 for centred a, b with S = sum a b^T: the eigenvector of the largest
// eigenvalue of Horn's matrix (the first maximum wins) as a quaternion, expanded in fp64
CBD_DEV void horn_rotation(const double (&S)[9], double (&R)[9]) {
  double N[4][4];
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  horn_matrix(S, N);
  jacobi_sweeps<true, false>(N, V);
  int best = 0;
  for (int k = 1; k < 4; ++k) if (N[k][k] > N[best][best]) best = k;
  const double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
  R[0] = w * w + x * x - y * y - z * z; R[1] = 2 * (x * y - w * z);           R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z);           R[4] = w * w - x * x + y * y - z * z; R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y);           R[7] = 2 * (y * z + w * x);           R[8] = w * w - x * x - y * y + z * z;
}

// largest eigenvalue of Horn's matrix: sum |R a - b|^2 = sum |a|^2 + sum |b|^2 - 2 lambda_max at the best rotation
CBD_DEV double horn_lambda_max(const double (&S)[9]) {
  double N[4][4];
  horn_matrix(S, N);
  jacobi_sweeps<false, true>(N, nullptr);
  return fmax(fmax(N[0][0], N[1][1]), fmax(N[2][2], N[3][3]));
}

// is every end of the R bonds E [R][2] an atom of a ligand of Nl atoms?  Wave vote, the same answer in every lane: what indexes LDS
// with a bond end asks this first.
CBD_DEV bool bond_ends_are_atoms(const int* __restrict__ E, int R, int Nl, int lane) {
  bool good = true;
  for (int r = lane; r < R; r += 64) {
    const int u = E[2 * r], v = E[2 * r + 1];
    good = good && u >= 0 && u < Nl && v >= 0 && v < Nl;
  }
  return __all(good) != 0;
}

// bit a of a packed mask_rotate row (one bit per atom, ceil(Nl / 32) words per bond)
CBD_DEV bool mask_bit(const unsigned* __restrict__ row, int a) { return (row[a >> 5] >> (a & 31)) & 1u; }

}  // namespace cbd
