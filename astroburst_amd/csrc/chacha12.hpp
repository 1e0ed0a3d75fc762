// The random stream of the synthetic generator (core/synth/*.rs): rand 0.8.5's StdRng = rand_chacha 0.3.1's ChaCha12Rng, seeded by
// rand_core 0.6.4's SeedableRng::seed_from_u64.  Written once for host and device code; no device memory, no HIP call.
//   key      eight little-endian u32 outputs of a PCG32 step over the 64-bit seed
//   state    "expand 32-byte k", the key, a 64-bit block counter (words 12, 13) that starts at 0, stream id 0 (words 14, 15)
//   output   the 16 words of block 0, then of block 1, ...; next_u64 = lo | hi << 32 of two consecutive words (the generator draws
//            u64s only, so pairs never straddle a block); gen::<f64>() = (next_u64() >> 11) as f64 * 2^-53
// Draw i of a stream is therefore words 2 i and 2 i + 1 of block i / 8: every index here is 64-bit (word 8 * pixel passes 2^32 at
// 2^29 pixels).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define AB_CC_HD __host__ __device__ __forceinline__
#else
#define AB_CC_HD inline
#endif

struct ab_chacha_key {
    uint32_t k[8];
};

AB_CC_HD ab_chacha_key ab_chacha_key_from_u64(uint64_t seed) {
    ab_chacha_key key;
    uint64_t state = seed;
    for (int i = 0; i < 8; ++i) {
        state = state * 6364136223846793005ull + 11634580027462260723ull;
        const uint32_t x = (uint32_t)(((state >> 18) ^ state) >> 27);
        const uint32_t rot = (uint32_t)(state >> 59);
        key.k[i] = (x >> rot) | (x << ((32u - rot) & 31u));
    }
    return key;
}

// (__builtin_rotateleft32 is one v_alignbit_b32 on gfx950)
#define AB_CC_QR(a, b, c, d)                     \
    do {                                         \
        a += b;                                  \
        d = __builtin_rotateleft32(d ^ a, 16);   \
        c += d;                                  \
        b = __builtin_rotateleft32(b ^ c, 12);   \
        a += b;                                  \
        d = __builtin_rotateleft32(d ^ a, 8);    \
        c += d;                                  \
        b = __builtin_rotateleft32(b ^ c, 7);    \
    } while (0)

// one 64-byte block: `rounds` is 12 for the generator (20 gives RFC 7539's block function with a 64-bit counter and a zero nonce)
template <int ROUNDS>
AB_CC_HD void ab_chacha_block(const ab_chacha_key &key, uint64_t counter, uint32_t out[16]) {
    const uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key.k[0], key.k[1], key.k[2], key.k[3],
                             key.k[4],    key.k[5],    key.k[6],    key.k[7],    (uint32_t)counter, (uint32_t)(counter >> 32), 0u, 0u};
    uint32_t x0 = in[0], x1 = in[1], x2 = in[2], x3 = in[3], x4 = in[4], x5 = in[5], x6 = in[6], x7 = in[7];
    uint32_t x8 = in[8], x9 = in[9], x10 = in[10], x11 = in[11], x12 = in[12], x13 = in[13], x14 = in[14], x15 = in[15];
#pragma unroll
    for (int r = 0; r < ROUNDS; r += 2) {
        AB_CC_QR(x0, x4, x8, x12);
        AB_CC_QR(x1, x5, x9, x13);
        AB_CC_QR(x2, x6, x10, x14);
        AB_CC_QR(x3, x7, x11, x15);
        AB_CC_QR(x0, x5, x10, x15);
        AB_CC_QR(x1, x6, x11, x12);
        AB_CC_QR(x2, x7, x8, x13);
        AB_CC_QR(x3, x4, x9, x14);
    }
    out[0] = x0 + in[0], out[1] = x1 + in[1], out[2] = x2 + in[2], out[3] = x3 + in[3];
    out[4] = x4 + in[4], out[5] = x5 + in[5], out[6] = x6 + in[6], out[7] = x7 + in[7];
    out[8] = x8 + in[8], out[9] = x9 + in[9], out[10] = x10 + in[10], out[11] = x11 + in[11];
    out[12] = x12 + in[12], out[13] = x13 + in[13], out[14] = x14 + in[14], out[15] = x15 + in[15];
}

// draw j (0 .. 7) of a block as gen::<f64>()
AB_CC_HD double ab_chacha_f64(const uint32_t w[16], int j) {
    const uint64_t u = (uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32);
    return (double)(u >> 11) * 0x1p-53;
}

// the serial view of a stream the host walks use: draw() returns draws `pos`, `pos + 1`, ... of the seed's stream
struct ab_chacha_stream {
    ab_chacha_key key;
    uint64_t pos = 0, have = ~0ull;  // `have`: the block in w (none yet)
    uint32_t w[16];
    explicit ab_chacha_stream(uint64_t seed, uint64_t skip = 0) : key(ab_chacha_key_from_u64(seed)), pos(skip) {}
    double draw() {
        const uint64_t b = pos >> 3;
        if (b != have) {
            ab_chacha_block<12>(key, b, w);
            have = b;
        }
        return ab_chacha_f64(w, (int)(pos++ & 7));
    }
};
