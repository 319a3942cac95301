// sample_key.h -- the sampling key of include/gnnagg.h ("Neighbour sampling"), one text for the device kernels (sample.hip) and the host
// sampler (host_graph.cpp).  murmur3's 32-bit finalizer, all arithmetic uint32 with wrap-around; a bijection of p for a fixed seed.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GNNAGG_HD __host__ __device__
#else
#define GNNAGG_HD
#endif

namespace gnnagg {

GNNAGG_HD static inline uint32_t sample_fmix(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// once per call
GNNAGG_HD static inline uint32_t sample_seed_mix(unsigned long long seed)
{
    return sample_fmix(sample_fmix((uint32_t)seed + 0x9E3779B9u) ^ (uint32_t)(seed >> 32));
}

// p: the edge's position in the full CSR
GNNAGG_HD static inline uint32_t sample_key(uint32_t p, uint32_t s) { return sample_fmix(sample_fmix(p ^ s) + s); }

}  // namespace gnnagg
