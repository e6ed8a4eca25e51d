// exact_float.hip.h -- float helpers that must not be contracted into fma: the reference is an x86-64 build without it, so a
// float expression that decides a boolean (box test, radius test, nearest-neighbour distance) rounds every step.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace dddmr {

// (HIP's __fmul_rn / __fadd_rn are plain operators compiled under the translation
// unit's -ffp-contract=fast, i.e. they still carry the `contract` flag and the
// backend may fuse them; the pragma below is what actually keeps them apart.)
__device__ __forceinline__ float fmul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float fadd(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float fsub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

// FLANN L2_Simple<float>: result = 0; result += diff*diff per dimension.
__device__ __forceinline__ float l2_simple(float ax, float ay, float az, float bx, float by, float bz) {
  float d = fsub(ax, bx);
  float r = fmul(d, d);
  d = fsub(ay, by);
  r = fadd(r, fmul(d, d));
  d = fsub(az, bz);
  r = fadd(r, fmul(d, d));
  return r;
}
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
  return fadd(fadd(fmul(ax, bx), fmul(ay, by)), fmul(az, bz));
}

}  // namespace dddmr
