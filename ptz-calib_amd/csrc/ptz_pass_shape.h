// ptz_pass_shape.h -- the grid extent of one LM pass of a scene group (plain host code: no HIP, no library state, so that a
// stand-alone harness can call it; tests/cpu_harness/pass_shape_harness.cc).
//
// A batch keeps a LADDER of launch shapes: entry 0 is the full-size shape (its extent is the group's scene count), the others are
// compacted shapes by ascending slot count.  The ladder decides two things only: which kernel variants and factorisation path a
// pass gets, and -- when passes are replayed from captured graphs, whose grids are frozen -- the grid extent.  A pass that is
// enqueued launch by launch can have any extent, so it gets exactly as many slots as scenes were last reported active, always
// through the device's compacted list once a single scene has retired: no workgroup exists for a scene that is known to be done.
#pragma once

namespace ptz {

struct PassExtent {
  int shape;     // index into the ladder: the variant fields of the pass come from this shape
  int slots;     // grid extent over scenes
  bool compact;  // slots index the device's compacted scene list
};

// count: the scenes the device last reported active (stale, hence an upper bound; any value is tolerated).  group_n: scenes of the
// group.  ladder[0 .. n_ladder): slot counts, [0] the full-size shape (value unused), [1..] ascending; n_ladder == 1: the batch
// keeps no compacted list at all.  graph: the pass is replayed from a captured graph.  exact_fit = false restores the ladder's
// extents for eagerly enqueued passes as well (A/B measurements).
inline PassExtent pass_extent(int count, int group_n, const int* ladder, int n_ladder, bool graph, bool exact_fit)
{
  PassExtent e;
  e.shape = 0;
  // the smallest compacted shape that covers the count; full size while none smaller than the group does
  for (int k = 1; k < n_ladder; ++k)
    if (ladder[k] >= count && ladder[k] < group_n) { e.shape = k; break; }
  e.slots = e.shape ? ladder[e.shape] : group_n;
  e.compact = e.shape != 0;
  if (graph || !exact_fit || n_ladder <= 1) return e;
  e.slots = count < 1 ? 1 : (count > group_n ? group_n : count);
  e.compact = e.slots < group_n;
  return e;
}

}  // namespace ptz
