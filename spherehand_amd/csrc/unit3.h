// unit3.h -- the unit normalisation of a three-vector with its zero rule (include/spherehand_hip.h, shr_tri_vertex_normals_fwd
// step 3), shared by tri_normals.hip and depth_normals.hip: one statement, one sequence of bits.
#pragma once
#include "common.h"

namespace shr {

constexpr float kNrmMaxFinite = 3.4028234663852886e38f;

// n = N / sqrt((Nx Nx + Ny Ny) + Nz Nz) with the IEEE root and three IEEE divisions; false (n = 0, nothing flows back)
// unless the sum of squares is positive and finite
__device__ __forceinline__ bool unit3(const float (&N)[3], float (&n)[3]) {
  const float s = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2];
  const bool live = s > 0.f && s <= kNrmMaxFinite;
  const float r = sqrtf(live ? s : 1.f);
#pragma unroll
  for (int d = 0; d < 3; d++) n[d] = live ? N[d] / r : 0.f;
  return live;
}

}  // namespace shr
