// Counter-keyed RANSAC sampling shared by the homography RANSAC (frontend.hip) and the pose RANSAC
// (pose_ransac.hip): the sampling stream is a function of (seed, hypothesis, draw, attempt) only, so any thread
// (or the host, or the NumPy oracle's _ransac_draw) reproduces a hypothesis' sample without shared state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptzba {

__device__ __host__ inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// draw k of hypothesis h: a function of (seed, h, k, attempt) only
__device__ __host__ inline uint32_t ransac_draw(uint64_t seed, uint32_t h, uint32_t k, uint32_t attempt, uint32_t n) {
  const uint64_t z = mix64(seed * 0x9E3779B97F4A7C15ull + ((uint64_t)h << 20) + ((uint64_t)attempt << 4) + k + 1);
  return (uint32_t)(z % n);
}

}  // namespace ptzba
