// usv_wrap_layout.hpp -- the mirrored frame ring of the fused wrappers (usv_wrap.hpp): where the frame
// of a step sits in an env's ring row, where the stacked observation begins, and which slots a done
// env clears.  Plain host C++ (no HIP), so the index rules are tested on their own
// (tests/test_wrap_layout.py); the kernels and the C ABI take them from here.
//
// One row per env, 2k - 1 slots of D floats (k = n_stack, D = obs_dim); no frame is ever shifted.
// Slots 0 .. k-1 are primaries: the frame of step counter j goes to slot p = j mod k.  Slots
// k .. 2k-2 are mirrors: slot q + k repeats primary q, for q <= k - 2.  After the frame of j is
// written, the k slots from s = (j + 1) mod k on hold the frames j-k+1 .. j, oldest first:
//   slots s .. k-1   primaries of the residues s .. k-1: the frames j-k+1 .. j-s (the newest of each
//                    residue, none of them rewritten since),
//   slots k .. s+k-1 mirrors of the residues 0 .. s-1: the frames j-s+1 .. j.
// s <= k - 1, so the window ends at slot 2k - 2 at most: the mirror of primary k - 1 would be slot
// 2k - 1, which no window reaches (with p = k - 1 the window is the primaries themselves), so that
// slot does not exist and the frame of such a step is written once.  That is the "one slot fewer" of
// the 2k-slot mirrored ring.  Every env shares j, so the stacked observation of all envs is one
// column window of the ring: a [N, k D] view, inner stride 1, row stride wrap_ring_stride.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace usv {

constexpr int wrap_ring_slots(int k) { return 2 * k - 1; }

// Floats per env row: the slots, rounded up to 4 floats so that every row starts at the 16-B phase of
// the ring's base.
constexpr size_t wrap_ring_stride(int D, int k) { return ((size_t)wrap_ring_slots(k) * (size_t)D + 3) / 4 * 4; }

// The slots the frame of step counter j (>= 0) is written to: the primary, and its mirror or -1.
constexpr int wrap_slot(int64_t j, int k) { return (int)(j % k); }
constexpr int wrap_mirror_slot(int64_t j, int k) { return wrap_slot(j, k) < k - 1 ? wrap_slot(j, k) + k : -1; }

// First slot, and first float within a row, of the stacked observation once frame j is written.
constexpr int wrap_window_slot(int64_t j, int k) { return (int)((j + 1) % k); }
constexpr size_t wrap_window_offset(int D, int k, int64_t j) { return (size_t)wrap_window_slot(j, k) * (size_t)D; }

// Whether slot q (0 <= q < wrap_ring_slots(k)) is zeroed when an env restarts at step counter j (done in
// the step of j, or reset at j): every copy of the frames before j, i.e. every slot but those of j.
// These are more than the k - 1 older slots of the window of j: the other copy of an older frame
// enters a later window.
constexpr bool wrap_clears_slot(int64_t j, int k, int q) { return q % k != wrap_slot(j, k); }

// The frames j-k+1 .. j-1 (the stack of a terminal observation without its last frame) before frame j
// is written: the window of j - 1 less its oldest frame, (k - 1) D contiguous floats from this slot on.
constexpr int wrap_terminal_slot(int64_t j, int k) { return wrap_slot(j, k) + 1; }

}  // namespace usv
