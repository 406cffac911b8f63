// The counter-based generator shared by the training feed (p2w_feed.hip) and the random subset (p2w_sample.hip); every user keeps a
// stream word of its own in counter word 3 (P2W_FEED_STREAM, P2W_SAMPLE_STREAM in include/p2w.h).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds, the key bumped by the
// Weyl constants between rounds
__device__ __forceinline__ void p2w_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned w[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
