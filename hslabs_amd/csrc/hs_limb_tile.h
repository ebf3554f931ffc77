// hs_limb_tile.h -- the slot sequence of the limb-lane kernel's tile mapping (hs_limb.h, TILE).
//
// A tile-mapped launch of n local steps gives every rollout the slot sequence: all even local steps
// ascending, then all odd ones. Tile t of a rollout is slots 8 t .. 8 t + 7, one slot per 8-lane group of
// the wavefront; slots past the sequence are idle groups (in the last tile only). Consecutive slots are
// two steps apart, so a group's stencil rows t - 2dt and t + 2dt are its neighbours' centre rows wherever
// the table row advances with the step (the kernel tests the rows themselves, not this sequence).
//
// Plain C++: host code, device code and a CPU test include it.
#pragma once

#if defined(__HIP__)
#define HS_TILE_FN __host__ __device__ inline
#else
#define HS_TILE_FN inline
#endif

constexpr int HS_TILE_SLOTS = 8;  // slots per tile: the 8-lane groups of a wavefront

// tiles of a launch of n local steps
HS_TILE_FN int limb_tile_count(int n) { return (n + HS_TILE_SLOTS - 1) / HS_TILE_SLOTS; }

// the local step of a slot, -1 for a slot past the sequence
HS_TILE_FN int limb_tile_step(int slot, int n) {
  const int n_even = (n + 1) / 2;
  if (slot < 0 || slot >= n) return -1;
  return slot < n_even ? 2 * slot : 2 * (slot - n_even) + 1;
}
