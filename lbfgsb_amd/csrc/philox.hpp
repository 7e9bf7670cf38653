// philox.hpp -- the counter-based generator behind lbfgsb_hip_qn_draw (k_qn_draw.hip), shared by host and device:
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123
// constants) and the map of its four output words to two uniforms.  Integer arithmetic and exact fp64 conversions
// only, so host and device give the same bits; the transcendental part of the normal deviates (log, sqrt, sinpi /
// cospi) is the caller's.
//
// A draw is a function of (seed, global row, sample index) alone:
//   counter = (row lo, row hi, pair lo, pair hi), row = the global 0-based row, pair = sample >> 1
//   key     = (seed lo, seed hi)
//   a = w0 2^32 + w1, b = w2 2^32 + w3;  u = ((a >> 12) + 0.5) 2^-52 in (0, 1),  v = (b >> 12) 2^-52 in [0, 1)
//   r = sqrt(-2 log u);  an even sample takes r cospi(2 v), an odd one r sinpi(2 v)
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LBP_HD __host__ __device__ __forceinline__
#else
#define LBP_HD inline
#endif

namespace lbp {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

// ten rounds; c: the counter in, the four output words out
LBP_HD void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)PHILOX_M0 * c[0], p1 = (uint64_t)PHILOX_M1 * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0, c[1] = (uint32_t)p1, c[2] = n2, c[3] = (uint32_t)p0;
    k0 += PHILOX_W0, k1 += PHILOX_W1;
  }
}

// the two uniforms of (seed, row, pair): u in (0, 1), v in [0, 1), both exact in fp64
LBP_HD void uniforms(uint64_t seed, uint64_t row, uint64_t pair, double &u, double &v) {
  uint32_t c[4] = {(uint32_t)row, (uint32_t)(row >> 32), (uint32_t)pair, (uint32_t)(pair >> 32)};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint64_t a = ((uint64_t)c[0] << 32) | c[1], b = ((uint64_t)c[2] << 32) | c[3];
  u = ((double)(a >> 12) + 0.5) * 0x1p-52;
  v = (double)(b >> 12) * 0x1p-52;
}

}  // namespace lbp
