// The digest launch of the transaction signer (hsv_signer_sign_transactions*,
// include/hsv.h; csrc/hsv_txsign.hpp): SHA-512(message)[..32] and the slot
// status of every transaction of a batch, into the launch workspace the
// signing launch (hsv_tx_sign_kernel, hsv_signer.hip) reads.
//
// One lane per transaction, the wave's loads staged through LDS exactly as the
// record kernel of the verifier loads (tx_record_lane, hsv_mempool.hip) -- that
// kernel itself cannot serve: it reads a pk and a signature that do not exist
// yet.  Nothing is handed between workgroups: an ordinary launch, followed on
// the same stream by the signing launch.
#include <hip/hip_runtime.h>

#define HSV_SHA_BITOP3 1  // v_bitop3_b32 in the message hash, as hsv_mempool.hip
#include "hsv_internal.h"
#include "hsv_stage.hpp"
#include "hsv_txsign.hpp"

namespace hsv {

constexpr int kTxDigestBlock = 256;
constexpr int kTxDigestWaves = kTxDigestBlock / 64;
constexpr int kTxDigestQ = 9;  // 16-B chunks under a 128-B window at any offset

// Each lane hashes its own blocks, the wave loops over its longest message, so
// the trip count is wave-uniform.  A lane past n redoes transaction n - 1 and
// stores nothing; every store sits after the loop.  Only a transaction that
// will be signed is loaded: a skipped one may have offsets that point anywhere.
__global__ void __launch_bounds__(kTxDigestBlock)
hsv_tx_digest_kernel(const uint8_t *__restrict__ txs, const uint64_t *__restrict__ offsets, uint64_t tx_size,
                     const uint32_t *__restrict__ key_idx, uint32_t nkeys, uint32_t n, uint4 *__restrict__ dig,
                     uint32_t *__restrict__ status) {
  __shared__ uint4 stage_all[kTxDigestWaves][64 * kTxDigestQ];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  if (blockIdx.x * kTxDigestBlock + wv * 64u >= n) return;  // whole wave past the end
  uint4 *stage = stage_all[wv];
  const uint32_t i_in = blockIdx.x * kTxDigestBlock + threadIdx.x;
  const uint32_t i = i_in < n ? i_in : n - 1u;
  uint64_t lo = 0, hi = 0;
  const bool span_ok = tx_sign_span(offsets, tx_size, i, lo, hi);
  const uint32_t st = tx_sign_status(span_ok, key_idx ? key_idx[i] : i, nkeys);
  const bool hash = st == kSlotOk;
  const uintptr_t base = reinterpret_cast<uintptr_t>(txs);
  const uint4 *q = reinterpret_cast<const uint4 *>(base & ~uintptr_t(15));
  const uint64_t start = hash ? (uint64_t)(base & 15u) + lo : 0;
  const uint64_t mlen = hash ? hi - lo - kTxTailBytes : 0;
  // the last chunk holding a byte of the transaction bounds every load
  const uint64_t q_last = hash ? (start + (hi - lo) - 1) >> 4 : kNoChunk;

  uint64_t h[8];
  sha512_init(h);
  const uint64_t nblocks = tx_num_blocks(mlen);
  uint32_t wave_blocks = (uint32_t)nblocks;
  HSV_UNROLL
  for (int m = 1; m < 64; m <<= 1) wave_blocks = max(wave_blocks, (uint32_t)__shfl_xor((int)wave_blocks, m, 64));
  const uint32_t sh16 = (uint32_t)(start & 15u);
  // wave-uniform fast paths: every transaction of the wave starts on a 16-byte
  // boundary (no realignment), and block b lies wholly inside every message
  // (no padding selects) -- the common case of equal-sized transactions
  const bool wave_aligned = __all(sh16 == 0u);
  HSV_NOUNROLL
  for (uint32_t b = 0; b < wave_blocks; ++b) {
    uint32_t raw[4 * kTxDigestQ + 1];
    tx_stage_chunks<kTxDigestQ>(q, stage, lane, (start >> 4) + 8ull * b, q_last, raw);
    const bool wave_full = __all((uint64_t)(b + 1u) * 128u <= mlen);
    if (b < nblocks) {
      uint32_t words[32];
      if (wave_aligned) {
        HSV_UNROLL
        for (int j = 0; j < 32; ++j) words[j] = raw[j];
      } else {
        tx_realign<32>(raw, sh16, words);
      }
      if (wave_full) tx_compress_full_block(h, words);
      else tx_compress_block(h, words, mlen, b, nblocks);
    }
  }
  uint32_t d[8];
  tx_digest_words(h, d);
  if (i_in < n) {
    dig[2 * (size_t)i] = make_uint4(d[0], d[1], d[2], d[3]);
    dig[2 * (size_t)i + 1] = make_uint4(d[4], d[5], d[6], d[7]);
    status[i] = st;
  }
}

}  // namespace hsv

// dig: n * 32 bytes (16-byte aligned), status: n words
extern "C" hipError_t hsv_launch_tx_digest(const uint8_t *txs, const uint64_t *offsets, uint64_t tx_size,
                                           const uint32_t *key_idx, uint32_t nkeys, uint32_t n, uint8_t *dig,
                                           uint32_t *status, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t grid = (n + hsv::kTxDigestBlock - 1) / hsv::kTxDigestBlock;
  hipLaunchKernelGGL(hsv::hsv_tx_digest_kernel, dim3(grid), dim3(hsv::kTxDigestBlock), 0, stream, txs, offsets,
                     tx_size, key_idx, nkeys, n, reinterpret_cast<uint4 *>(dig), status);
  return hipGetLastError();
}
