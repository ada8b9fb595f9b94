// shf_quat.h -- the quaternion product the controllers' orientation errors share (shf_glue.hip: k_ik_dls, k_osc; shf_qp.hip).
#pragma once
#include <hip/hip_runtime.h>

static __device__ __forceinline__ void shf_quat_mul(const float* a, const float* b, float* o) {   // torch_utils.py:12-33 (xyzw)
  const float x1 = a[0], y1 = a[1], z1 = a[2], w1 = a[3], x2 = b[0], y2 = b[1], z2 = b[2], w2 = b[3];
  const float ww = (z1 + x1) * (x2 + y2);
  const float yy = (w1 - y1) * (w2 + z2);
  const float zz = (w1 + y1) * (w2 - z2);
  const float xx = ww + yy + zz;
  const float qq = 0.5f * (xx + (z1 - x1) * (x2 - y2));
  o[3] = qq - ww + (z1 - y1) * (y2 - z2);
  o[0] = qq - xx + (x1 + w1) * (x2 + w2);
  o[1] = qq - yy + (w1 - x1) * (y2 + z2);
  o[2] = qq - zz + (z1 + y1) * (w2 - x2);
}
