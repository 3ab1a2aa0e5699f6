// The items of a host batch and how a staged call walks them.  Pure host
// arithmetic: no HIP include, builds with plain g++ (tests/native/batch_host.cpp).
//
// A batch is ragged -- item i is bytes [offsets[i], offsets[i + 1]) of the
// caller's buffer, n + 1 non-decreasing offsets -- or fixed: item i is `len`
// bytes at i * stride (stride 0: every item is the same `len` bytes).
// hsv_verify_transactions*, hsv_verify_msgs, hsv_signer_sign_transactions and
// hsv_signer_sign_msgs stage such a batch chunk by chunk: at most max_items items and max_bytes
// bytes per launch, an item larger than max_bytes alone in its chunk.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace hsvh {

struct BatchSpan {
  const uint64_t *offsets;  // NULL: the fixed form
  size_t stride, len;       // the fixed form (ignored when offsets != NULL)

  // End b > a of the chunk that starts at item a < n (max_items >= 1).  A fixed
  // item counts as `stride` bytes; stride 0 is bounded by max_items alone.
  size_t chunk_end(size_t a, size_t n, size_t max_items, size_t max_bytes) const {
    if (!offsets) {
      const size_t per = stride ? std::min(max_items, std::max<size_t>(1, max_bytes / stride)) : max_items;
      return std::min(n, a + per);
    }
    size_t b = a + 1;
    while (b < n && b - a < max_items && offsets[b + 1] - offsets[a] <= max_bytes) ++b;
    return b;
  }
  // First byte of item a in the caller's buffer.
  size_t first_byte(size_t a) const { return offsets ? (size_t)offsets[a] : a * stride; }
  // Bytes from the first byte of item a to the last byte of item b - 1 (b > a).
  size_t span_bytes(size_t a, size_t b) const {
    return offsets ? (size_t)(offsets[b] - offsets[a]) : (b - a - 1) * stride + len;
  }
  // The b - a + 1 offsets of a ragged chunk relative to its first byte:
  // rel[0] = 0, rel[b - a] = span_bytes(a, b).
  void rel_offsets(size_t a, size_t b, uint64_t *rel) const {
    for (size_t k = 0; k <= b - a; ++k) rel[k] = offsets[a + k] - offsets[a];
  }
};

// First i < n whose offsets decrease or whose item is shorter than min_len
// bytes; n when there is none.
inline size_t first_bad_item(const uint64_t *offsets, size_t n, uint64_t min_len) {
  for (size_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] < min_len) return i;
  return n;
}

}  // namespace hsvh
