// Device helpers of the pose arithmetic shared by pose_update_kernel (kernels.hip) and noise_conformers_kernel (noise_transform.hip):
// the quaternion route from an axis-angle vector to its rotation matrix and the 64-lane butterfly sums.  Moved here from kernels.hip
// word for word, so that both kernels run the same instructions.
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

}  // namespace cbd
