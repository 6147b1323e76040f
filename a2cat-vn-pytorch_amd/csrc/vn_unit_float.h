// vn_unit_float.h — ScaledFloatFrame's arithmetic for one byte: float(u8) / 255.0f as IEEE
// fp32 division, bit for bit, without a division. Compiles for the device (vn_env.hip's float
// observation tail) and for the host (tests/test_float_obs.py checks all 256 values).
//
// u * fl(1/255) alone differs from u / 255 in the last bit for 126 of the 256 byte values.
// One correction step on the quotient repairs it: with q0 = fl(u * r), the residual
// e = u - 255 q0 comes exactly out of one fma, and fl(q0 + e r) is the correctly rounded
// quotient for every byte value (there are only 256: the test compares them all, bitwise,
// with np.float32(u) / np.float32(255)).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VN_UNIT_FN __host__ __device__ __forceinline__
#else
#define VN_UNIT_FN inline
#endif

namespace vn {

// u: a byte value already converted to float (0.0f .. 255.0f, integral)
VN_UNIT_FN float unit_from_byte_value(float u) {
  const float r = 1.0f / 255.0f;  // a constant: fl(1/255)
  const float q = u * r;
  const float e = fmaf(-q, 255.0f, u);
  return fmaf(e, r, q);
}

VN_UNIT_FN float unit_from_u8(uint8_t b) { return unit_from_byte_value((float)b); }

}  // namespace vn
