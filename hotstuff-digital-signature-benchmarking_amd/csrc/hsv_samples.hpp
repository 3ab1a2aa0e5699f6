// The benchmark's sample transactions (node/src/client.rs:106-148 and the
// `benchmark` block of BatchMaker::seal, mempool/src/batch_maker.rs:118-125),
// host and device: which transaction of a burst is the sample, what its first
// nine bytes are, and which transaction of a batch seal() reports as one.
// hsv_samples.hip runs this on the device, hsv_samples_api.cpp on the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HSV_SM_FN __host__ __device__ __forceinline__
#else
#define HSV_SM_FN inline
#endif

namespace hsv {

constexpr uint32_t kSamplesTile = 256;   // transactions per workgroup of the index kernels
constexpr uint32_t kClientGroup = 16;    // lanes per transaction of the burst kernel
constexpr uint64_t kClientPreamble = 9;  // tag byte and a big-endian u64

// seal()'s filter: tx[0] == 0 && tx.len() > 8 (an empty transaction, on which
// the reference's tx[0] would panic, is not a sample)
HSV_SM_FN bool is_sample(uint64_t len, uint8_t first) { return len > 8u && first == 0u; }

HSV_SM_FN uint64_t samples_bswap64(uint64_t v) {
  v = ((v & 0x00ff00ff00ff00ffull) << 8) | ((v >> 8) & 0x00ff00ff00ff00ffull);
  v = ((v & 0x0000ffff0000ffffull) << 16) | ((v >> 16) & 0x0000ffff0000ffffull);
  return (v << 32) | (v >> 32);
}

// The standard (non-sample) transactions among the first m of a client that
// starts at burst counter counter0: every whole burst holds burst - 1 of them
// (its sample sits at position counter % burst < burst), the open burst the x
// transactions before m less its sample if that came first.  Mod 2^64.
HSV_SM_FN uint64_t client_standard_before(uint64_t m, uint64_t burst, uint64_t counter0) {
  const uint64_t j = m / burst, x = m % burst;
  const uint64_t s = (counter0 + j) % burst;
  return j * (burst - 1u) + x - (s < x ? 1u : 0u);
}

// The first 16 bytes of a transaction as two little-endian words: tag, BE64(v), zeros.
struct ClientPreamble {
  uint64_t lo, hi;
  // bytes [p, p + 16) of the transaction, p < 16 (the bytes past 8 are zero)
  HSV_SM_FN void from(uint32_t p, uint64_t &a, uint64_t &b) const {
    const uint32_t s = 8u * (p & 7u);
    if (p >= 8u) {
      a = hi >> s;
      b = 0;
    } else {
      a = s ? (lo >> s) | (hi << (64u - s)) : lo;
      b = hi >> s;
    }
  }
  // byte p of the transaction, any p below the zero padding's end
  HSV_SM_FN uint8_t byte(uint64_t p) const {
    return p < 8u ? (uint8_t)(lo >> (8u * p)) : p == 8u ? (uint8_t)hi : (uint8_t)0;
  }
};

// transaction i of the call (client.rs:121-133): the sample of its burst
// carries 0 and the burst counter, any other 1 and the running r
HSV_SM_FN ClientPreamble client_preamble(uint64_t i, uint64_t burst, uint64_t counter0, uint64_t r0) {
  const uint64_t c = counter0 + i / burst, x = i % burst;
  const bool sample = x == c % burst;
  const uint64_t v = samples_bswap64(sample ? c : r0 + client_standard_before(i + 1u, burst, counter0));
  return {(sample ? 0ull : 1ull) | (v << 8), v >> 56};
}

}  // namespace hsv
