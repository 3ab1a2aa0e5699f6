// Host (CPU) build of the message signer's per-lane code (csrc/hsv_msgsign.hpp
// over csrc/hsv_sign_core.hpp and csrc/hsv_msghash.hpp), for
// tests/test_msgsign_host.py.  Test infrastructure: the product library never
// signs with this code on the CPU.
//
//   msgsign_host --group      prints G of the product launches
//   msgsign_host --sign       stdin: batches
//        M <base> <m> <msg_len | -1> <msg_stride> <inject_item | -1> <nkeys> <use_idx 0|1> <nbytes>
//        <seed_hex>                 (nkeys lines)
//        I <idx> ...                (use_idx: m key indices)
//        O <off> ...                (msg_len -1: m + 1 offsets relative to the buffer)
//        D <hex | ->                (nbytes bytes: the messages)
//     The message bytes go to byte `base` of a 16-byte aligned allocation of
//     exactly the 16-byte lines they touch (none at all, and a NULL pointer,
//     when nbytes is 0), so a read past the last line is out of bounds.  Keys
//     are expanded and the three launches run the way the kernels do: the nonce
//     of every item first (msg_nonce_item), then the points in waves of 64
//     lanes, lane l of wave w carrying items w*64*G + g*64 + l (sign_lane with
//     MsgSignIo; item inject_item reads a zeroed table entry), then every
//     item's response (msg_response_item).  Prints the m * 64 signature
//     bytes, "guards 0|1" (1: the 0xa5 bytes around the signature array are
//     intact) and "fault 0|1".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "hsv_msgsign.hpp"

using namespace hsv;

static const uint32_t kBaseY[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u,
                                   0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};

// the narrow comb: the same lane code as the kernels' wide one, a table that
// takes a fraction of the time to build here
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

static bool parse_hex(const std::string &s, std::vector<uint8_t> &out) {
  out.clear();
  if (s == "-") return true;
  if (s.size() % 2) return false;
  out.reserve(s.size() / 2);
  auto nib = [](char c) -> int {
    return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
  };
  for (size_t i = 0; i < s.size(); i += 2) {
    const int hi = nib(s[i]), lo = nib(s[i + 1]);
    if (hi < 0 || lo < 0) return false;
    out.push_back((uint8_t)(hi * 16 + lo));
  }
  return true;
}

static void print_hex(const uint8_t *p, size_t n) {
  static const char *d = "0123456789abcdef";
  std::string s(2 * n, '0');
  for (size_t i = 0; i < n; ++i) {
    s[2 * i] = d[p[i] >> 4];
    s[2 * i + 1] = d[p[i] & 15];
  }
  fputs(s.c_str(), stdout);
}

// the launch workspace of one lane: G slots of kSignWsWords words
struct HostStore {
  uint32_t *w;
  void put(int g, int i, uint32_t v) { w[g * kSignWsWords + i] = v; }
  uint32_t get(int g, int i) const { return w[g * kSignWsWords + i]; }
};

template <typename T>
static bool read_list(const char *tag, size_t count, std::vector<T> &out) {
  std::string line, t;
  if (!std::getline(std::cin, line)) return false;
  std::istringstream is(line);
  if (!(is >> t) || t != tag) return false;
  out.resize(count);
  for (size_t i = 0; i < count; ++i)
    if (!(is >> out[i])) return false;
  return true;
}

constexpr size_t kGuard = 64;

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  constexpr int G = kSignGroup;
  if (mode == "--group") {
    printf("%d\n", G);
    return 0;
  }
  if (mode != "--sign") return 2;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream is(line);
    std::string tag;
    long long base, m, msg_len, msg_stride, inject_item, nkeys, use_idx, nbytes;
    if (!(is >> tag >> base >> m >> msg_len >> msg_stride >> inject_item >> nkeys >> use_idx >> nbytes) || tag != "M" ||
        base < 0 || base > 15 || m < 1)
      return 2;
    std::vector<uint8_t> seeds((size_t)nkeys * 32 + 16), keys((size_t)nkeys * 96 + 16);
    for (long long i = 0; i < nkeys; ++i) {
      std::vector<uint8_t> sb;
      if (!std::getline(std::cin, line) || !parse_hex(line, sb) || sb.size() != 32) return 2;
      memcpy(seeds.data() + 32 * i, sb.data(), 32);
    }
    std::vector<uint32_t> idx;
    std::vector<uint64_t> offs;
    if (use_idx && !read_list("I", (size_t)m, idx)) return 2;
    if (msg_len < 0 && !read_list("O", (size_t)m + 1, offs)) return 2;
    std::vector<uint8_t> data;
    {
      std::string t, hex;
      if (!std::getline(std::cin, line)) return 2;
      std::istringstream id(line);
      if (!(id >> t >> hex) || t != "D" || !parse_hex(hex, data) || (long long)data.size() != nbytes) return 2;
    }
    // exactly the 16-byte lines the messages touch
    const size_t chunks = data.empty() ? 0 : ((size_t)base + data.size() + 15) / 16;
    uint8_t *lines = chunks ? static_cast<uint8_t *>(aligned_alloc(16, 16 * chunks)) : nullptr;
    const uint8_t *msgs = nullptr;
    if (chunks) {
      memset(lines, 0xa5, 16 * chunks);
      memcpy(lines + base, data.data(), data.size());
      msgs = lines + base;
    }
    const uint32_t base16 = chunks ? (uint32_t)base : 0u;
    auto ld = [&](uint64_t k, uint32_t w[4]) {
      if (k >= chunks) { fprintf(stderr, "load past the messages\n"); exit(3); }
      memcpy(w, lines + 16 * k, 16);
    };
    std::vector<uint8_t> sigmem(kGuard + (size_t)m * 64 + kGuard + 16, 0xa5);
    uint8_t *sigblk = sigmem.data() + ((16 - (reinterpret_cast<uintptr_t>(sigmem.data()) & 15u)) & 15u);
    uint8_t *sig = sigblk + kGuard;

    const uint32_t *table = comb8_b();
    const uint32_t *key_idx = use_idx ? idx.data() : nullptr;
    const uint64_t *offsets = msg_len < 0 ? offs.data() : nullptr;
    const uint64_t len = msg_len < 0 ? 0 : (uint64_t)msg_len;
    uint32_t bad = 0;
    std::vector<uint32_t> ws((size_t)G * kSignWsWords);
    HostStore st{ws.data()};
    {
      KeygenArgs ka{seeds.data(), (uint64_t)nkeys, keys.data(), table, kInjectNone, 0};
      for (uint64_t wave = 0; wave * 64 * G < ka.n; ++wave)
        for (uint32_t lane = 0; lane < 64; ++lane) bad |= keygen_lane<8, G>(ka, wave * 64 * G + lane, 64, st);
    }
    // the nonce launch
    std::vector<uint32_t> nonce((size_t)m * 8), status((size_t)m);
    for (long long i = 0; i < m; ++i)
      msg_nonce_item(ld, base16, keys.data(), (uint32_t)nkeys, key_idx, offsets, len, (uint64_t)msg_stride, (uint64_t)i,
                     nonce.data() + 8 * i, status[i]);
    // the point launch
    {
      SignArgs sa{keys.data(), (uint32_t)nkeys, key_idx, nullptr, 0, 0, (uint64_t)m, sig, 64, table,
                  inject_item >= 0 ? (uint32_t)kInjectZeroTables : (uint32_t)kInjectNone,
                  (uint32_t)(inject_item >= 0 ? inject_item : 0)};
      const MsgSignIo io{status.data(), reinterpret_cast<const uint8_t *>(nonce.data())};
      for (uint64_t wave = 0; wave * 64 * G < sa.m; ++wave)
        for (uint32_t lane = 0; lane < 64; ++lane) bad |= sign_lane<8, G, false>(sa, wave * 64 * G + lane, 64, st, io);
    }
    // the response launch
    for (long long i = 0; i < m; ++i)
      msg_response_item(ld, base16, keys.data(), key_idx, offsets, len, (uint64_t)msg_stride, (uint64_t)i,
                        reinterpret_cast<const uint8_t *>(nonce.data()), status.data(), sig, 64);
    print_hex(sig, (size_t)m * 64);
    printf("\n");
    int guards = 1;
    for (size_t k = 0; k < kGuard; ++k)
      if (sigblk[k] != 0xa5 || sig[(size_t)m * 64 + k] != 0xa5) guards = 0;
    printf("guards %d\nfault %u\n", guards, bad);
    free(lines);
  }
  return 0;
}
