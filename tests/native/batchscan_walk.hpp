// The device walk of a serialized batch (csrc/hsv_batchscan.hpp) run on the
// host exactly as hsv_batchwire.hip's wave runs it: the batch placed at a given
// misalignment inside a chunk stream, one window of kScanWindow bytes at a
// time, only the chunks that hold a byte of the batch copied in, everything
// else -- the bytes around the batch inside its first and last chunk, the
// window's unloaded tail and its slack words -- filled with a pattern the walk
// must never interpret.  Shared by batchscan_host.cpp and batch_wire_fuzz.cpp.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "hsv_batchscan.hpp"

namespace bsw {

struct Walked {
  bool ok = false;
  uint64_t count = 0, windows = 0;
  std::vector<uint64_t> spans;  // 2 per transaction, relative to the batch
};

inline Walked walk(const uint8_t *buf, size_t len, uint32_t mis, uint8_t fill) {
  Walked out;
  // the stream: mis pattern bytes, the batch, pattern up to the chunk's end
  std::vector<uint8_t> stream(((size_t)mis + len + 15) / 16 * 16, fill);
  if (len) std::memcpy(stream.data() + mis, buf, len);
  hsv::BatchWalk wk;
  wk.begin(len, mis);
  const uint64_t nwin = wk.windows();
  std::vector<uint32_t> win(hsv::kScanWindow / 4 + hsv::kScanSlackWords);
  for (uint64_t k = 0; k < nwin && !wk.done(); ++k, ++out.windows) {
    std::memset(win.data(), fill, win.size() * 4);
    const size_t lo = (size_t)k * hsv::kScanWindow;
    const size_t n = stream.size() > lo ? stream.size() - lo : 0;
    std::memcpy(win.data(), stream.data() + lo, n < hsv::kScanWindow ? n : hsv::kScanWindow);
    wk.window(win.data(), k, [&](uint64_t i, uint64_t a, uint64_t e) {
      if (i * 2 != out.spans.size()) out.spans.push_back(~0ull);  // out of order: shows as a mismatch
      out.spans.push_back(a);
      out.spans.push_back(e);
    });
  }
  out.ok = wk.ok();
  out.count = wk.ok() ? wk.count : 0;
  if (!wk.done()) out.windows = ~0ull;  // the walk must end within windows()
  return out;
}

}  // namespace bsw
