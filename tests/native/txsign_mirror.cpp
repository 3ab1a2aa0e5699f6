// A caller of hsv::Signer::sign_transactions (include/hsv_crypto.hpp), for
// tests/test_txsign_cpp.py: a client signs its transactions in place and the
// mempool's check accepts them.
//   txsign_mirror            signs, verifies, prints "all passed"
// Without a GPU the constructor throws crypto::InfrastructureError (there is no
// CPU fallback), which main reports on stderr with exit status 3.
#include <cstdio>
#include <cstring>
#include <vector>

#include "hsv_crypto.hpp"

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

static int run() {
  constexpr size_t kKeys = 5, kSize = 113;  // 17 message bytes: neighbours share words
  std::vector<std::array<uint8_t, 32>> seeds(kKeys);
  for (size_t i = 0; i < kKeys; ++i)
    for (size_t j = 0; j < 32; ++j) seeds[i][j] = (uint8_t)(31 * i + 7 * j + 1);
  hsv::Signer signer(seeds);
  CHECK(signer.size() == kKeys);

  // equal transactions, item i with key i
  std::vector<uint8_t> txs(kKeys * kSize, 0xCC);
  for (size_t i = 0; i < kKeys; ++i)
    for (size_t j = 0; j < kSize - 96; ++j) txs[i * kSize + j] = (uint8_t)(i * 17 + j);
  const std::vector<uint8_t> before = txs;
  signer.sign_transactions(txs, kSize);
  std::vector<uint8_t> flags(kKeys);
  CHECK(hsv_verify_transactions_fixed(txs.data(), kSize, kKeys, flags.data()) == HSV_OK);
  for (size_t i = 0; i < kKeys; ++i) {
    uint8_t pk[32];
    CHECK(hsv_public_key(seeds[i].data(), pk) == HSV_OK);
    CHECK(flags[i] & HSV_STRICT_OK);
    CHECK(memcmp(txs.data() + i * kSize, before.data() + i * kSize, kSize - 96) == 0);  // the message is the caller's
    CHECK(memcmp(txs.data() + (i + 1) * kSize - 96, pk, 32) == 0);
  }

  // ragged, keys by index; an index past the keys leaves 96 zero bytes
  const uint64_t offsets[4] = {0, 96, 96 + 200, 96 + 200 + 97};
  const uint32_t idx[3] = {4, 0, 5};
  std::vector<uint8_t> rag(offsets[3], 0x11);
  signer.sign_transactions(idx, rag.data(), offsets, 0, 3);
  CHECK(hsv_verify_transactions(rag.data(), offsets, 3, flags.data()) == HSV_OK);
  CHECK((flags[0] & HSV_STRICT_OK) && (flags[1] & HSV_STRICT_OK) && !(flags[2] & HSV_STRICT_OK));
  for (size_t j = 0; j < 96; ++j) CHECK(rag[offsets[3] - 96 + j] == 0);
  CHECK(rag[offsets[2]] == 0x11);

  // a transaction shorter than 96 bytes throws, and nothing is written
  std::vector<uint8_t> small(95 * 2, 0x22);
  bool threw = false;
  try {
    signer.sign_transactions(small, 95);
  } catch (const crypto::InfrastructureError &) {
    threw = true;
  }
  CHECK(threw && small == std::vector<uint8_t>(95 * 2, 0x22));
  printf("all passed\n");
  return 0;
}

int main() {
  try {
    return run();
  } catch (const crypto::InfrastructureError &e) {
    fprintf(stderr, "InfrastructureError: %s\n", e.what());
    return 3;
  }
}
