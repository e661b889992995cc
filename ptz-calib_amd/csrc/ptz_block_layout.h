// ptz_block_layout.h -- how one device block is cut into 256-byte aligned slots.  Plain C++, no HIP: the host check of the layouts
// (tests/cpu_harness/krt_batch_layout_harness.cc) compiles this file and ptz_krt_batch_layout.h on their own.
#pragma once

#include <cstddef>

namespace ptz {

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// the cursor: take(bytes) is the offset of the next slot, total() the bytes taken so far
struct BlockLayout {
  size_t at = 0;
  size_t take(size_t bytes) { const size_t o = at; at += up256(bytes); return o; }
  size_t total() const { return at; }
};

}  // namespace ptz
