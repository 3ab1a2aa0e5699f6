// A caller of hsv::Signer::sign_msgs (include/hsv_crypto.hpp), for
// tests/test_msgsign_cpp.py: a load generator signs messages of differing
// lengths in one call, the host signer agrees byte for byte and the message
// verifier accepts them.
//   msgsign_mirror            signs, compares, verifies, prints "all passed"
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
  constexpr size_t kKeys = 6;
  const size_t lens[kKeys] = {0, 1, 47, 80, 176, 1023};  // empty, and block-count changes of both hashes
  std::vector<std::array<uint8_t, 32>> seeds(kKeys);
  for (size_t i = 0; i < kKeys; ++i)
    for (size_t j = 0; j < 32; ++j) seeds[i][j] = (uint8_t)(29 * i + 5 * j + 3);
  hsv::Signer signer(seeds);
  CHECK(signer.size() == kKeys);

  // one message per item, item i with key i
  std::vector<std::vector<uint8_t>> msgs(kKeys);
  std::vector<uint8_t> buf, pk(kKeys * 32);
  std::vector<uint64_t> offsets(1, 0);
  for (size_t i = 0; i < kKeys; ++i) {
    for (size_t j = 0; j < lens[i]; ++j) msgs[i].push_back((uint8_t)(i * 13 + j));
    buf.insert(buf.end(), msgs[i].begin(), msgs[i].end());
    offsets.push_back(buf.size());
    CHECK(hsv_public_key(seeds[i].data(), pk.data() + 32 * i) == HSV_OK);
  }
  const std::vector<uint8_t> sig = signer.sign_msgs(msgs);
  CHECK(sig.size() == kKeys * 64);
  for (size_t i = 0; i < kKeys; ++i) {
    uint8_t want[64];
    CHECK(hsv_sign(seeds[i].data(), msgs[i].data(), msgs[i].size(), want) == HSV_OK);
    CHECK(memcmp(sig.data() + 64 * i, want, 64) == 0);
  }
  std::vector<uint8_t> flags(kKeys);
  CHECK(hsv_verify_msgs(pk.data(), sig.data(), buf.data(), offsets.data(), 0, 0, kKeys, flags.data()) == HSV_OK);
  for (size_t i = 0; i < kKeys; ++i) CHECK(flags[i] & HSV_STRICT_OK);

  // keys by index, a fixed stride; an index past the keys leaves 64 zero bytes
  const uint32_t idx[3] = {5, 0, 6};
  const std::vector<uint8_t> fixed = signer.sign_msgs(idx, buf.data(), nullptr, 33, 40, 3);
  uint8_t want[64];
  CHECK(hsv_sign(seeds[5].data(), buf.data(), 33, want) == HSV_OK && memcmp(fixed.data(), want, 64) == 0);
  CHECK(hsv_sign(seeds[0].data(), buf.data() + 40, 33, want) == HSV_OK && memcmp(fixed.data() + 64, want, 64) == 0);
  for (size_t j = 0; j < 64; ++j) CHECK(fixed[128 + j] == 0);

  // decreasing offsets throw
  const uint64_t down[3] = {0, 40, 30};
  bool threw = false;
  try {
    signer.sign_msgs(nullptr, buf.data(), down, 0, 0, 2);
  } catch (const crypto::InfrastructureError &) {
    threw = true;
  }
  CHECK(threw);
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
