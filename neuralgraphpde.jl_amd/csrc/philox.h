// philox.h -- the counter-based generator under the random graph operations (sampling.hip, graph_edit.hip): one definition, so every
// file that draws evaluates the same bits.
//
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), stateless: a value is a pure function of
// (seed, stream, counter) -- never of the thread, the launch geometry or the call order -- so a call gives the same bits on every
// run and a test restates the generator in numpy.  The streams are listed in include/ngpde.h (RANDOMNESS).
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace ngpde {

enum { kStreamNeighbor = 1, kStreamReplace = 2, kStreamSplit = 3, kStreamNegative = 4, kStreamLanczos = 5 };

// counter (c0, c1, stream, 0), key (lo32(seed), hi32(seed)); the 64-bit draw is out[0] | out[1] << 32
__device__ __forceinline__ unsigned long long philox_draw(unsigned long long seed, uint32_t stream, uint32_t c0, uint32_t c1) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t x0 = c0, x1 = c1, x2 = stream, x3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, x0), lo0 = 0xD2511F53u * x0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, x2), lo1 = 0xCD9E8D57u * x2;
    x0 = hi1 ^ x1 ^ k0;
    x1 = lo1;
    x2 = hi0 ^ x3 ^ k1;
    x3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return (unsigned long long)x0 | ((unsigned long long)x1 << 32);
}

}  // namespace ngpde
