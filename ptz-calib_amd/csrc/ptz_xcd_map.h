// ptz_xcd_map.h -- which item of a 2-D launch a workgroup takes, so that the 8 XCDs share the LIVE part of the launch evenly
// (plain index arithmetic for host and device: no HIP types, no library state, so that a stand-alone harness can call it;
// tests/cpu_harness/xcd_map_harness.cc).
//
// Workgroups are dealt round-robin over the 8 XCDs by linear id L = bx + gx * by.  A launch of gx x rows workgroups (x = item,
// y = scene slot) of which only rows 0 .. live-1 have work -- a pass through the device's compacted scene list, whose grid the
// host sized from an older, larger count -- gives XCD x = L % 8 the x-th of eight contiguous ranges of the gx x live item space,
// lengths differing by at most one; the workgroups idx = L / 8 beyond the range's length have nothing to do.  Every XCD thus gets
// an eighth of the work whatever the launch's extent, and the workgroups that share a scene's data still share one XCD's L2.
// The accepted ids map one-to-one onto [0, gx * live) whatever the hardware's real placement is: placement is a speed matter
// only, results never depend on it.  live == rows is the mapping of a launch without idle rows (every id accepted).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PTZ_XCD_HD __host__ __device__
#else
#define PTZ_XCD_HD
#endif

namespace ptz {

constexpr unsigned XCD_COUNT = 8;

struct XcdItem {
  bool work;        // false: this workgroup returns at once
  unsigned bx, by;  // the item (bx < gx, by < live) it takes
};

// L: linear workgroup id (< gx * rows for some rows >= live); gx >= 1.
PTZ_XCD_HD inline XcdItem xcd_live_item(unsigned L, unsigned gx, unsigned live)
{
  const unsigned total = gx * live;
  const unsigned q = total / XCD_COUNT, r = total % XCD_COUNT, xcd = L % XCD_COUNT, idx = L / XCD_COUNT;
  const unsigned len = q + (xcd < r ? 1u : 0u);
  const unsigned start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  XcdItem it;
  it.work = idx < len;
  const unsigned Lp = start + idx;
  it.bx = Lp % gx;
  it.by = Lp / gx;
  return it;
}

}  // namespace ptz
