// Host (CPU) build of the transaction signer's per-lane code (csrc/hsv_txsign.hpp
// over csrc/hsv_sign_core.hpp and csrc/hsv_txhash.hpp), for
// tests/test_txsign_host.py.  Test infrastructure: the product library never
// signs with this code on the CPU.
//
//   txsign_host --group      prints G of the product launches
//   txsign_host --tail       stdin lines "<base> <hex of 96 bytes>": tx_store_tail
//                            at byte `base` of a 16-byte aligned 0xa5 buffer;
//                            prints the 16 + 96 + 32 bytes around the store
//   txsign_host --sign       stdin: batches
//        T <base> <m> <tx_size | 0> <inject_item | -1> <nkeys> <use_idx 0|1> <nbytes>
//        <seed_hex>                 (nkeys lines)
//        I <idx> ...                (use_idx: m key indices)
//        O <off> ...                (tx_size 0: m + 1 offsets relative to the buffer)
//        D <hex | ->                (nbytes bytes: the transactions, tails unsigned)
//     The bytes go to byte 16 + base of a 16-byte aligned allocation filled
//     with 0xa5.  Keys are expanded, digests taken (tx_digest_item, every item
//     of the batch first, as the digest launch) and the tails signed the way
//     the kernels do it: waves of 64 lanes, lane l of wave w carrying items
//     w*64*G + g*64 + l; item inject_item reads a zeroed table entry.  Prints
//     the buffer, "guards 0|1" (1: every other byte of the allocation is
//     still 0xa5) and "fault 0|1".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "hsv_txsign.hpp"

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

static uint8_t *aligned_block(std::vector<uint8_t> &mem, size_t bytes) {
  mem.assign(bytes + 16, 0xa5);
  return mem.data() + ((16 - (reinterpret_cast<uintptr_t>(mem.data()) & 15u)) & 15u);
}

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

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  constexpr int G = kSignGroup;
  if (mode == "--group") {
    printf("%d\n", G);
    return 0;
  }
  std::string line;
  if (mode == "--tail") {
    while (std::getline(std::cin, line)) {
      std::istringstream is(line);
      size_t base;
      std::string hex;
      std::vector<uint8_t> b, mem;
      if (!(is >> base >> hex) || !parse_hex(hex, b) || b.size() != 96 || base > 31) return 2;
      uint8_t *blk = aligned_block(mem, 16 + 96 + 32);
      uint32_t w[24];
      for (int i = 0; i < 24; ++i)
        w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
               ((uint32_t)b[4 * i + 3] << 24);
      tx_store_tail(blk + 16 + base, w);
      print_hex(blk, 16 + 96 + 32);
      printf("\n");
    }
    return 0;
  }
  if (mode != "--sign") return 2;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream is(line);
    std::string tag;
    long long base, m, tx_size, inject_item, nkeys, use_idx, nbytes;
    if (!(is >> tag >> base >> m >> tx_size >> inject_item >> nkeys >> use_idx >> nbytes) || tag != "T" || base < 0 ||
        base > 15)
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
    if (tx_size == 0 && !read_list("O", (size_t)m + 1, offs)) return 2;
    std::vector<uint8_t> data, mem;
    {
      std::string t, hex;
      if (!std::getline(std::cin, line)) return 2;
      std::istringstream id(line);
      if (!(id >> t >> hex) || t != "D" || !parse_hex(hex, data) || (long long)data.size() != nbytes) return 2;
    }
    const size_t total = 16 + (size_t)base + data.size() + 16 + 16;  // guard | base | transactions | guard | slack
    uint8_t *blk = aligned_block(mem, total);
    uint8_t *txs = blk + 16 + base;
    if (!data.empty()) memcpy(txs, data.data(), data.size());

    const uint32_t *table = comb8_b();
    const uint32_t *key_idx = use_idx ? idx.data() : nullptr;
    const uint64_t *offsets = tx_size == 0 ? offs.data() : nullptr;
    uint32_t bad = 0;
    std::vector<uint32_t> ws((size_t)G * kSignWsWords);
    HostStore st{ws.data()};
    {
      KeygenArgs ka{seeds.data(), (uint64_t)nkeys, keys.data(), table, kInjectNone, 0};
      for (uint64_t wave = 0; wave * 64 * G < ka.n; ++wave)
        for (uint32_t lane = 0; lane < 64; ++lane) bad |= keygen_lane<8, G>(ka, wave * 64 * G + lane, 64, st);
    }
    // the digest launch: every item's digest and status before any tail is written
    std::vector<uint32_t> dig((size_t)m * 8 + 8), status((size_t)m + 1);
    {
      const uint8_t *q = blk + 16;  // txs rounded down to 16 bytes
      const size_t chunks = ((size_t)base + data.size() + 15) / 16;
      auto ld = [&](uint64_t k, uint32_t w[4]) {
        if (k >= chunks) { fprintf(stderr, "load past the transactions\n"); exit(3); }
        memcpy(w, q + 16 * k, 16);
      };
      for (long long i = 0; i < m; ++i)
        status[i] = tx_digest_item(ld, (uint32_t)base, offsets, (uint64_t)tx_size, key_idx, (uint32_t)nkeys, (uint64_t)i,
                                   dig.data() + 8 * i);
    }
    // the signing launch
    {
      SignArgs sa{keys.data(), (uint32_t)nkeys, key_idx, reinterpret_cast<const uint8_t *>(dig.data()), 32, 32,
                  (uint64_t)m, nullptr, 0, table,
                  inject_item >= 0 ? (uint32_t)kInjectZeroTables : (uint32_t)kInjectNone,
                  (uint32_t)(inject_item >= 0 ? inject_item : 0)};
      const TxSignIo io{status.data(), txs, offsets, (uint64_t)tx_size};
      for (uint64_t wave = 0; wave * 64 * G < sa.m; ++wave)
        for (uint32_t lane = 0; lane < 64; ++lane) bad |= sign_lane<8, G, true>(sa, wave * 64 * G + lane, 64, st, io);
    }
    print_hex(txs, data.size());
    printf("\n");
    int guards = 1;
    for (uint8_t *p = blk; p < blk + total; ++p)
      if ((p < txs || p >= txs + data.size()) && *p != 0xa5) guards = 0;
    printf("guards %d\nfault %u\n", guards, bad);
  }
  return 0;
}
