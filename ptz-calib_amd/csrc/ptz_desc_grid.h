// ptz_desc_grid.h -- the contract of the grid-binned guided matcher (k_desc_top2_guided_grid, ptz_desc_match_pairs_guided_grid): a
// second implementation of the guided contract of ptz_desc_match.h.  The admissible set, the rules over it and the output arrays are
// that header's, bit for bit; this one only says WHICH candidates a query tests and how a top-2 is kept when they arrive in no order.
//
// PTZ_HD like ptz_desc_match.h: the kernel and the host (tests/cpu_harness/desc_grid_harness.cc) instantiate the same functions.
//
// The frame.  One per (pair, direction, slab of the searched side): (x0, y0) the lower corner of the bounding box of the slab's
// FINITE searched positions, G x G cells of size c = max(r', extent / G) per axis, r' = desc_grid_reach(radius_px).  A slab
// without a finite position has an empty index.  The index holds the slab's finite positions sorted by cell = cy * G + cx, so the
// cells cx0 .. cx1 of one grid row are one contiguous run.
//
// The cell function.  desc_grid_cell(f, axis, v) = (int)clamp((v - origin) * (1 / c), 0, G - 1), all in double, the clamp BEFORE
// the conversion (NaN and -inf go to 0, 1e30 and +inf to G - 1: no undefined conversion).  It is ONE function of a coordinate and it
// is monotone non-decreasing in v: a rounded subtraction of a constant, a rounded product with a positive constant, a clamp and a
// truncation are each monotone.  It is applied to a candidate's coordinate and to a query's bounds q - r', q + r' alike; the search
// range of a query is [cell(q - r'), cell(q + r')] per axis.
//
// Why the range is conservative.  Let a candidate at c be admissible for the query at q (both float; one axis, d = c - q in reals).
//   * The predicate is e2 = fl(fl(dx dx) + fl(dy dy)) <= r2f in float, dx = fl(q - c), r2f = fl32(fl64(r r)).  fl(a + b) >= a for
//     b >= 0, so fl(dx dx) <= r2f <= r^2 (1 + 2^-24)(1 + 2^-53); a float product is within a factor (1 + 2^-24) of the real one or,
//     where it underflows, within 2^-150 of it; and dx = fl(q - c) is within a factor (1 + 2^-24) of d (a float difference never
//     underflows).  Together |d| <= r (1 + 2^-21) + 2^-74 in real numbers.
//   * r' = max(radius_px, 2^-60) (1 + 2^-10) is larger than that bound (the floor 2^-60 pays for the underflow term; it can only
//     widen a range).  So q - r' < c < q + r' in real numbers.
//   * c is a float, hence a double: rounding q - r' to double cannot carry it past c (rounding is monotone and c is representable),
//     so fl64(q - r') <= c <= fl64(q + r') -- nothing else is rounded between q -+ r' and the cell function, and no bound on the size
//     of the coordinates is needed.
//   * Monotonicity: cell(fl64(q - r')) <= cell(c) <= cell(fl64(q + r')), per axis.
// The grid only chooses who is TESTED: a tested candidate is admissible iff desc_guide_err2(...) <= r2f, the bits of
// ptz_desc_match.h.  A NaN position is never admissible; a searched position that is not finite is not indexed, a query that is not
// finite does not search (with a finite r2f neither can be admissible: its error is inf or NaN).  A radius whose r2f is not finite
// admits every pair whose error is not NaN, infinite positions included: the host runs the scan kernel for it.
//
// The order-free update.  desc_top2_take_keyed(T, d2, j) is desc_top2_merge(T, desc_top2_one(d2, j)): the best is the minimum
// under desc_key_less, the second the smallest d2 over the others.  Its result does not depend on the order of the candidates, so
// slabs, cells and the placement order inside a cell may be anything.
#pragma once

#include "ptz_desc_match.h"

namespace ptz {

#ifndef PTZ_DESC_GRID_G  // (-D overrides: A/B probe builds only; 16, 32 or 64 and 2048 or 4096)
#define PTZ_DESC_GRID_G 32
#endif
#ifndef PTZ_DESC_GRID_SLAB
#define PTZ_DESC_GRID_SLAB 2048
#endif
constexpr int kDescGridG = PTZ_DESC_GRID_G;          // cells per axis
constexpr int kDescGridSlab = PTZ_DESC_GRID_SLAB;    // searched positions indexed at a time (S)

struct DescGridFrame {
  double x0, y0;  // lower corner of the finite positions' bounding box
  double ix, iy;  // 1 / cell size, per axis
  bool empty;     // no finite position: nothing is indexed, nobody searches
};

PTZ_HD double desc_grid_reach(double radius_px)
{
  const double r = radius_px > 0x1p-60 ? radius_px : 0x1p-60;
  return r * (1.0 + 0x1p-10);
}

PTZ_HD bool desc_grid_indexed(float x, float y) { return desc_finite((double)x) && desc_finite((double)y); }

// the frame of positions whose finite ones span [xmin, xmax] x [ymin, ymax] (xmin > xmax: there is none)
PTZ_HD DescGridFrame desc_grid_frame(float xmin, float xmax, float ymin, float ymax, double reach)
{
  DescGridFrame f;
  f.empty = !(xmin <= xmax && ymin <= ymax);
  f.x0 = f.empty ? 0.0 : (double)xmin;
  f.y0 = f.empty ? 0.0 : (double)ymin;
  const double ex = f.empty ? 0.0 : ((double)xmax - (double)xmin) / kDescGridG;
  const double ey = f.empty ? 0.0 : ((double)ymax - (double)ymin) / kDescGridG;
  f.ix = 1.0 / (ex > reach ? ex : reach);
  f.iy = 1.0 / (ey > reach ? ey : reach);
  return f;
}

PTZ_HD int desc_grid_cell(const DescGridFrame& f, int axis, double v)
{
  double t = axis ? (v - f.y0) * f.iy : (v - f.x0) * f.ix;
  t = t > 0.0 ? t : 0.0;  // (a NaN goes to 0)
  t = t < (double)(kDescGridG - 1) ? t : (double)(kDescGridG - 1);
  return (int)t;
}

// a query's cells: [cx0, cx1] x [cy0, cy1]
struct DescGridRange {
  int cx0, cx1, cy0, cy1;
};

PTZ_HD DescGridRange desc_grid_range(const DescGridFrame& f, float qx, float qy, double reach)
{
  DescGridRange r;
  r.cx0 = desc_grid_cell(f, 0, (double)qx - reach);
  r.cx1 = desc_grid_cell(f, 0, (double)qx + reach);
  r.cy0 = desc_grid_cell(f, 1, (double)qy - reach);
  r.cy1 = desc_grid_cell(f, 1, (double)qy + reach);
  return r;
}

PTZ_HD void desc_top2_take_keyed(DescTop2& T, int32_t d2, int32_t j)
{
  const bool first = desc_key_less(d2, j, T.d, T.j);
  T.s = desc_min(T.s, first ? T.d : d2);
  T.j = first ? j : T.j;
  T.d = first ? d2 : T.d;
}

}  // namespace ptz
