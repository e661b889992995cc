// ptz_host_batch.h -- what one call of an entry point holds on the device until it returns, the owner of a pooled block that
// outlives a call, and the check every *_device entry point makes of the caller's buffers.  (The layout of a block is
// ptz_block_layout.h: up256 and the cursor.)
#pragma once

#include <utility>

#include "ptz_common.h"
#include "ptz_pool.h"
#include "ptz_block_layout.h"

namespace ptz {

// One pooled device block, optionally a pinned host block of the same size, a stream and the timing events around the launches.
// The stream is the pool's (default constructor: taken by acquire(), given back) or the caller's (waited on, never released).
// Whatever way the call returns, the destructor first waits for the stream and then gives everything back.
struct CallHeld {
  int dev = 0;
  char* base = nullptr;
  void* pinned = nullptr;
  hipStream_t st = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // acquire() takes two; the third is third_event()'s
  const bool pooled_stream;
  CallHeld() : pooled_stream(true) {}
  explicit CallHeld(hipStream_t callers) : st(callers), pooled_stream(false) {}
  CallHeld(const CallHeld&) = delete;
  CallHeld& operator=(const CallHeld&) = delete;
  ~CallHeld()
  {
    if (st || !pooled_stream) (void)stream_wait(st);
    release_blocks();
    if (pooled_stream) ptzpool::stream_release(dev, st);
    for (hipEvent_t e : ev) ptzpool::event_release(dev, true, e);
  }
  // The stream, if it is the pool's, and two events, unless the call holds them already: all a call without a block needs.
  int open(int device)
  {
    dev = device;
    if (pooled_stream && !st) PTZ_HIP_TRY(ptzpool::stream_acquire(dev, &st));
    for (int k = 0; k < 2; ++k)
      if (!ev[k]) PTZ_HIP_TRY(ptzpool::event_acquire(dev, true, &ev[k]));
    return PTZ_OK;
  }
  // A block of `bytes` -- blocks of an earlier acquire() go back first -- with a pinned one beside it if want_pinned (`pinned` stays
  // null, and the error is cleared, where the host has none to give), then open().  PTZ_ENOMEM: no device block (hipGetLastError()
  // is left to the caller).  Other failures as PTZ_HIP_TRY answers them.
  int acquire(int device, size_t bytes, bool want_pinned = false)
  {
    dev = device;
    release_blocks();
    if (ptzpool::dev_acquire(dev, bytes, (void**)&base) != hipSuccess) return PTZ_ENOMEM;
    if (want_pinned && ptzpool::pinned_acquire(bytes, &pinned) != hipSuccess) { pinned = nullptr; (void)hipGetLastError(); }
    return open(device);
  }
  hipError_t third_event() { return ptzpool::event_acquire(dev, true, &ev[2]); }
  // milliseconds between ev[from] and ev[from + 1], both recorded and reached
  double elapsed_ms(int from = 0) const
  {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ev[from], ev[from + 1]);
    return ms;
  }

 private:
  void release_blocks()
  {
    ptzpool::dev_release(dev, base);
    ptzpool::pinned_release(pinned);
    base = nullptr; pinned = nullptr;
  }
};

// A pooled device block that outlives the call that fills it (a descriptor set, a match table, a chunk's matches): it goes back to
// the pool with its owner.  The owner must outlive any CallHeld whose stream writes the block -- declare it first -- so that the
// stream has been waited for when the block goes back.  Movable (a vector of parts), not copyable.
struct PoolBlock {
  int dev = 0;
  char* p = nullptr;
  PoolBlock() = default;
  PoolBlock(PoolBlock&& o) noexcept : dev(o.dev), p(std::exchange(o.p, nullptr)) {}
  ~PoolBlock() { ptzpool::dev_release(dev, p); }
  hipError_t get(int device, size_t bytes) { dev = device; return ptzpool::dev_acquire(dev, bytes, (void**)&p); }
};

// The device that owns `p`, checked against the stream's: a launch goes to the device that owns the caller's buffers, on the caller's
// stream -- a caller holding tensors and a stream on GPU 1 must not need to say so again.  PTZ_OK or the error to return.
inline int owning_device(const void* p, void* hip_stream, int* device)
{
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PTZ_ENODEVICE;
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return PTZ_EINVAL; }
  *device = attr.device;
  if (hip_stream) {
    hipDevice_t sdev = -1;
    if (hipStreamGetDevice((hipStream_t)hip_stream, &sdev) != hipSuccess) { (void)hipGetLastError(); return PTZ_EINVAL; }
    if ((int)sdev != *device) return PTZ_EINVAL;  // stream and buffers live on different devices
  }
  if (*device < 0 || *device >= ndev) return PTZ_EINVAL;
  return PTZ_OK;
}

}  // namespace ptz
