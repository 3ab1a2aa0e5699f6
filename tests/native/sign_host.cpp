// Host (CPU) build of the signing kernels' per-lane core (csrc/hsv_sign_core.hpp),
// for tests/test_sign_host.py.  Test infrastructure: the product library never
// signs with this code on the CPU (hsv_sign_many is its host signer).
//
//   sign_host --group            prints G of the product launches
//   sign_host --comb             stdin lines "WB scalar_hex" (32 bytes, little-endian);
//                                prints compress([x]B) per line
//   sign_host --sign             stdin: batches
//        B <wb> <msg_len> <m> <inject_item | -1> <grouped 0|1>
//        <seed_hex> <msg_hex | ->          (m lines)
//     keys are expanded and messages signed the way the kernels do it: waves of
//     64 lanes, lane l of wave w carrying items w*64*G + g*64 + l (g < G), with
//     G = the product's group (grouped = 1) or 1; item inject_item reads a
//     zeroed table entry.  Prints "pk_hex sig_hex" per item, then "fault 0|1".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "hsv_sign_core.hpp"

using namespace hsv;

static const uint32_t kBaseY[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u,
                                   0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};

static const uint32_t *comb8_b() {
  static std::vector<uint32_t> tab;
  if (tab.empty()) {
    tab.resize(kCombTableWords);
    std::vector<uint32_t> tmp(kCombEnt * 8);
    fe x, y;
    ge_decompress(kBaseY, x, y);
    for (int j = 0; j < kCombPos; ++j)
      comb_build_position(comb_position_base(x, y, 0, j), tab.data() + (uint64_t)j * kCombEnt * kCombEntryWords,
                          tmp.data());
  }
  return tab.data();
}

static const uint32_t *comb16_b() {
  static std::vector<uint32_t> tab;
  if (tab.empty()) {
    tab.resize(kComb16TableWords);
    std::vector<uint32_t> tmp(kComb16Chunk * 8);
    fe x, y;
    ge_decompress(kBaseY, x, y);
    for (int j = 0; j < kComb16Pos; ++j)
      for (uint32_t c = 0; c < (uint32_t)kComb16ChunksPerPos; ++c) comb16_build_chunk(x, y, j, c, tab.data(), tmp.data());
  }
  return tab.data();
}

static bool parse_hex(const std::string &s, std::vector<uint8_t> &out) {
  out.clear();
  if (s == "-") return true;
  if (s.size() % 2) return false;
  for (size_t i = 0; i < s.size(); i += 2) {
    unsigned v;
    if (sscanf(s.c_str() + i, "%2x", &v) != 1) return false;
    out.push_back((uint8_t)v);
  }
  return true;
}

static void print_hex(const uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
}

// the launch workspace of one lane: G slots of kSignWsWords words
struct HostStore {
  uint32_t *w;
  void put(int g, int i, uint32_t v) { w[g * kSignWsWords + i] = v; }
  uint32_t get(int g, int i) const { return w[g * kSignWsWords + i]; }
};

template <int WB, int G>
static uint32_t run_keygen(const KeygenArgs &a) {
  std::vector<uint32_t> ws((size_t)G * kSignWsWords);
  HostStore st{ws.data()};
  uint32_t bad = 0;
  for (uint64_t wave = 0; wave * 64 * G < a.n; ++wave)
    for (uint32_t lane = 0; lane < 64; ++lane) bad |= keygen_lane<WB, G>(a, wave * 64 * G + lane, 64, st);
  return bad;
}

template <int WB, int G>
static uint32_t run_sign(const SignArgs &a) {
  std::vector<uint32_t> ws((size_t)G * kSignWsWords);
  HostStore st{ws.data()};
  uint32_t bad = 0;
  for (uint64_t wave = 0; wave * 64 * G < a.m; ++wave)
    for (uint32_t lane = 0; lane < 64; ++lane)
      bad |= a.msg_len == 32 ? sign_lane<WB, G, true>(a, wave * 64 * G + lane, 64, st)
                             : sign_lane<WB, G, false>(a, wave * 64 * G + lane, 64, st);
  return bad;
}

template <int WB>
static uint32_t run_batch(KeygenArgs &ka, SignArgs &sa, bool grouped) {
  uint32_t bad = grouped ? run_keygen<WB, kSignGroup>(ka) : run_keygen<WB, 1>(ka);
  bad |= grouped ? run_sign<WB, kSignGroup>(sa) : run_sign<WB, 1>(sa);
  return bad;
}

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "--group") {
    printf("%d\n", kSignGroup);
    return 0;
  }
  std::string line;
  if (mode == "--comb") {
    while (std::getline(std::cin, line)) {
      std::istringstream is(line);
      int wb;
      std::string hex;
      std::vector<uint8_t> b;
      if (!(is >> wb >> hex) || !parse_hex(hex, b) || b.size() != 32 || (wb != 8 && wb != 16)) return 2;
      uint32_t x[8], enc[8];
      sign_load16<8>(b.data(), x);
      ge_compress(wb == 16 ? fixed_base_comb<16>(x, comb16_b()) : fixed_base_comb<8>(x, comb8_b()), enc);
      uint8_t out[32];
      sign_store16<8>(out, enc);
      print_hex(out, 32);
      printf("\n");
    }
    return 0;
  }
  if (mode != "--sign") return 2;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream is(line);
    std::string tag;
    int wb, grouped;
    long long msg_len, m, inject_item;
    if (!(is >> tag >> wb >> msg_len >> m >> inject_item >> grouped) || tag != "B" || (wb != 8 && wb != 16)) return 2;
    std::vector<uint8_t> seeds((size_t)m * 32 + 16), msgs((size_t)m * msg_len + 16), keys((size_t)m * 96 + 16),
        sigs((size_t)m * 64 + 16);
    for (long long i = 0; i < m; ++i) {
      std::string sh, mh;
      std::vector<uint8_t> sb, mb;
      if (!std::getline(std::cin, line)) return 2;
      std::istringstream it(line);
      if (!(it >> sh >> mh) || !parse_hex(sh, sb) || !parse_hex(mh, mb) || sb.size() != 32 || (long long)mb.size() != msg_len)
        return 2;
      memcpy(seeds.data() + 32 * i, sb.data(), 32);
      if (msg_len) memcpy(msgs.data() + msg_len * i, mb.data(), msg_len);
    }
    const uint32_t *table = wb == 16 ? comb16_b() : comb8_b();
    KeygenArgs ka{seeds.data(), (uint64_t)m, keys.data(), table, kInjectNone, 0};
    SignArgs sa{keys.data(), (uint32_t)m, nullptr, msgs.data(), (uint64_t)msg_len, (uint64_t)msg_len, (uint64_t)m,
                sigs.data(), 64, table, inject_item >= 0 ? (uint32_t)kInjectZeroTables : (uint32_t)kInjectNone,
                (uint32_t)(inject_item >= 0 ? inject_item : 0)};
    const uint32_t bad = wb == 16 ? run_batch<16>(ka, sa, grouped != 0) : run_batch<8>(ka, sa, grouped != 0);
    for (long long i = 0; i < m; ++i) {
      print_hex(keys.data() + 96 * i + 64, 32);
      printf(" ");
      print_hex(sigs.data() + 64 * i, 64);
      printf("\n");
    }
    printf("fault %u\n", bad);
  }
  return 0;
}
