// ptz_desc_set.h -- what a resident descriptor set is (ptz_desc_set_create, ptz_desc_match.hip), for the files whose kernels read
// one: the matcher and the shortlist.  Rows are packed as ptz_desc_match.hip describes: a byte xor 0x80 as int8, rows padded with
// zeros to 64 KS bytes, every image to a multiple of DESC_ROW_PAD rows (zero rows, norm INT32_MAX), and DESC_ROW_PAD such rows of
// slack behind the last image.
#pragma once

#include <algorithm>
#include <vector>

#include "ptz_common.h"
#include "ptz_pool.h"

namespace ptz {

constexpr int DESC_ROW_PAD = 64;  // rows of an image are padded to this

// a call's stream and timing events, from the pool
struct DescStream {
  int dev = 0;
  hipStream_t st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t open(int device)
  {
    dev = device;
    hipError_t e = ptzpool::stream_acquire(dev, &st);
    if (e == hipSuccess) e = ptzpool::event_acquire(dev, true, &e0);
    if (e == hipSuccess) e = ptzpool::event_acquire(dev, true, &e1);
    return e;
  }
  ~DescStream()
  {
    if (st) (void)stream_wait(st);
    ptzpool::stream_release(dev, st);
    ptzpool::event_release(dev, true, e0);
    ptzpool::event_release(dev, true, e1);
  }
};
struct DescBlock {  // a pooled device block, released with its owner
  int dev = 0;
  char* p = nullptr;
  hipError_t get(int device, size_t bytes) { dev = device; return ptzpool::dev_acquire(dev, std::max<size_t>(bytes, 256), (void**)&p); }
  ~DescBlock() { ptzpool::dev_release(dev, p); }
  DescBlock() = default;
  DescBlock(const DescBlock&) = delete;
  DescBlock& operator=(const DescBlock&) = delete;
};

}  // namespace ptz

struct ptz_desc_set {
  int device = 0;
  int32_t n_img = 0, D = 0, KS = 0;
  int64_t n_feat = 0;
  std::vector<int64_t> feat_ptr, row_off;  // [n_img + 1]
  ptz::DescBlock blk;
  int8_t* d_desc = nullptr;   // [rows + slack][64 KS]
  int32_t* d_norm = nullptr;  // [rows + slack]
  float2* d_kp = nullptr;     // [n_feat] or nullptr
  // the two offset tables on the device as well, [n_img + 2]: entry n_img + 1 closes the slack (feat_ptr: no features)
  const int64_t* d_feat_ptr = nullptr;
  const int64_t* d_row_off = nullptr;
};
