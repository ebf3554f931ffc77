// hs_limb_tile.h -- the slot sequence of the limb-lane kernel's tile mapping (hs_limb.h, TILE).
//
// Tile t of a rollout is slots 8 t .. 8 t + 7 of the launch's slot sequence, one slot per 8-lane group of
// the wavefront; slots past the sequence are idle groups (in the last tile only). A group's stencil rows
// t - 2dt and t + 2dt are its neighbours' centre rows wherever consecutive slots hold steps whose table
// rows are 2 apart (decided from the rows themselves, not the sequence, so any sequence gives the same
// values). Every row no neighbour holds is a request (limb_tile_kd); the first E0 of a tile run beside the
// centre rows, every further eight cost the wavefront one more FK pass. The host decides all this once per
// launch and hands it to the kernel as the tile descriptor (limb_tile_desc).
//
// Two sequences:
//   the parity order (limb_tile_step): all even local steps ascending, then all odd ones. Consecutive
//     slots are two steps apart, but the table row wraps with the gait period (n_t = 20: every 10 slots),
//     and a wrap inside a tile is a break: 2 more requests.
//   the plan (limb_tile_plan): the launch's steps cut into chains whose rows ascend by 2, every run of 8
//     of a chain a tile of its own (2 requests), the chains' remainders packed into the remaining tiles
//     with as few segments per tile as the greedy finds. Kept only where it needs fewer passes than the
//     parity order under limb_tile_passes, the kernel's own request arithmetic.
// Every sequence holds each local step in exactly one slot, fills limb_tile_count(n) tiles, has its idle
// slots (-1) at the end of the last tile only, and so a live slot 0 in every tile.
//
// The tile loop: a wavefront runs a chunk of consecutive tiles of its rollout (limb_tile_chunks).
//
// Plain C++ without allocation: host code, device code and the CPU tests include it.
#pragma once

#include <stdint.h>

#if defined(__HIP__)
#define HS_TILE_FN __host__ __device__ inline
#else
#define HS_TILE_FN inline
#endif

constexpr int HS_TILE_SLOTS = 8;  // slots per tile: the 8-lane groups of a wavefront

// tiles of a launch of n local steps
HS_TILE_FN int limb_tile_count(int n) { return (n + HS_TILE_SLOTS - 1) / HS_TILE_SLOTS; }

// the parity order: the local step of a slot, -1 for a slot past the sequence
HS_TILE_FN int limb_tile_step(int slot, int n) {
  const int n_even = (n + 1) / 2;
  if (slot < 0 || slot >= n) return -1;
  return slot < n_even ? 2 * slot : 2 * (slot - n_even) + 1;
}

// ---- the tile loop ----
// A wavefront runs tl consecutive tiles of its rollout, one after the other (launch_map::limb_tile_loop):
// the launch's nt tiles are cut into chunks of tl, the last one shorter when tl does not divide nt. tl = 1
// is a tile per wavefront (chunk c = tile c); a tl below 1 counts as 1.
HS_TILE_FN int limb_tile_chunks(int nt, int tl) {
  tl = tl < 1 ? 1 : tl;
  return (nt + tl - 1) / tl;
}
// chunk c runs tiles [limb_tile_chunk_first, limb_tile_chunk_end) in order
HS_TILE_FN int limb_tile_chunk_first(int c, int tl) { return c * (tl < 1 ? 1 : tl); }
HS_TILE_FN int limb_tile_chunk_end(int c, int tl, int nt) {
  const int e = limb_tile_chunk_first(c, tl) + (tl < 1 ? 1 : tl);
  return e < nt ? e : nt;
}

// The routing rule's arithmetic (limb_tile_loop() in hs_capi.cpp): `tiles` tiles per wavefront, fewer while
// the launch's chunks x rollouts stay under min_waves wavefronts in its queue, and the tiles then spread
// evenly over the chunks that remain (5 tiles in 2 chunks: 3 + 2, not 4 + 1)
HS_TILE_FN int limb_tile_loop_rule(int nt, int64_t n_rollouts, int tiles, int64_t min_waves) {
  int tl = tiles < nt ? tiles : nt;
  while (tl > 1 && (int64_t)limb_tile_chunks(nt, tl) * n_rollouts < min_waves) tl--;
  if (tl < 1) return 1;
  const int nc = limb_tile_chunks(nt, tl);
  return (nt + nc - 1) / nc;
}

// ---- the plan ----
constexpr int HS_TILE_PLAN_STEPS = 256;  // the longest launch a plan holds (HS_FUSED_MAX_STEPS' default)

// a launch as the planner sees it: n local steps from global step s0 of calls of h steps, the call's
// k0 and n_t, and the limb lanes of a group (the launch's largest model)
struct limb_tile_launch {
  int n, s0, h, k0, n_t, n_limbs;
};

// the table row of a local step as hs_limb_kernel forms it, less the launch's constant ktab_lo
HS_TILE_FN int limb_tile_row(const limb_tile_launch& L, int step) {
  const int s_glob = L.s0 + step, call = s_glob / L.h;
  return (int)(((int64_t)L.k0 + (int64_t)call * L.h) % L.n_t) + s_glob % L.h;
}
// row[i] = limb_tile_row(L, i) of the launch's n steps
HS_TILE_FN void limb_tile_rows(const limb_tile_launch& L, int* row) {
  for (int i = 0; i < L.n; i++) row[i] = limb_tile_row(L, i);
}

// requests the first pass serves on the lanes idle in every group (limb_tile_kd's E0)
HS_TILE_FN int limb_tile_e0(int n_limbs) {
  return n_limbs > 0 && n_limbs < HS_TILE_SLOTS ? HS_TILE_SLOTS * (HS_TILE_SLOTS - n_limbs) / n_limbs : 0;
}

// limb_tile_kd's requests of one tile (row[]: the launch's limb_tile_rows), bit 2 g slot g's minus row,
// bit 2 g + 1 its plus row: a live slot's minus (plus) row is shared only with the live slot before (after)
// it in the tile whose row is exactly 2 lower (higher); every other one is a request
HS_TILE_FN uint32_t limb_tile_request_mask(const int* row, const int16_t* slots) {
  uint32_t M = 0;
  for (int g = 0; g < HS_TILE_SLOTS; g++) {
    if (slots[g] < 0) continue;
    const int r = row[slots[g]];
    const bool shm = g > 0 && slots[g - 1] >= 0 && row[slots[g - 1]] + 2 == r;
    const bool shp = g < HS_TILE_SLOTS - 1 && slots[g + 1] >= 0 && row[slots[g + 1]] == r + 2;
    M |= (uint32_t)!shm << (2 * g) | (uint32_t)!shp << (2 * g + 1);
  }
  return M;
}
HS_TILE_FN int limb_tile_requests(const int* row, const int16_t* slots) { return __builtin_popcount(limb_tile_request_mask(row, slots)); }

// the further FK passes of a tile with `req` requests, and of a launch's whole sequence
HS_TILE_FN int limb_tile_req_passes(int req, int n_limbs) {
  const int over = req - limb_tile_e0(n_limbs);
  return over > 0 ? (over + HS_TILE_SLOTS - 1) / HS_TILE_SLOTS : 0;
}
HS_TILE_FN int limb_tile_passes(const int* row, int n, int n_limbs, const int16_t* step) {
  int passes = 0;
  for (int t = 0; t < limb_tile_count(n); t++)
    passes += limb_tile_req_passes(limb_tile_requests(row, step + HS_TILE_SLOTS * t), n_limbs);
  return passes;
}
HS_TILE_FN int limb_tile_passes(const limb_tile_launch& L, const int16_t* step) {  // (n <= HS_TILE_PLAN_STEPS)
  int row[HS_TILE_PLAN_STEPS];
  limb_tile_rows(L, row);
  return limb_tile_passes(row, L.n, L.n_limbs, step);
}

// step[8 * limb_tile_count(n)] = the parity order
HS_TILE_FN void limb_tile_parity_fill(int n, int16_t* step) {
  for (int s = 0; s < HS_TILE_SLOTS * limb_tile_count(n); s++) step[s] = (int16_t)limb_tile_step(s, n);
}

// step[8 * limb_tile_count(n)] = the chain-aligned sequence (1 <= n <= HS_TILE_PLAN_STEPS): every run of
// 8 of a chain in a tile of its own, in chain order; then the remainders (1 .. 7 steps each), a tile at a
// time: the longest that still fits until the tile is full, and where none fits the head of the shortest
// one left (a split, only to keep the tile count)
HS_TILE_FN void limb_tile_chain_fill(const int* row, int n, int16_t* step) {
  const int n_slots = HS_TILE_SLOTS * limb_tile_count(n);
  // the remainders, listed by length in chain order: first step rem0[], the next of the same length nxt[]
  // (a record per remainder and per split, at most one split a tile)
  constexpr int NREC = HS_TILE_PLAN_STEPS + HS_TILE_PLAN_STEPS / HS_TILE_SLOTS;
  int16_t rem0[NREC], nxt[NREC];
  int head[HS_TILE_SLOTS], tail[HS_TILE_SLOTS], n_rem = 0, out = 0;
  for (int k = 0; k < HS_TILE_SLOTS; k++) head[k] = tail[k] = -1;
  auto push = [&](int first, int len) {
    rem0[n_rem] = (int16_t)first;
    nxt[n_rem] = -1;
    if (tail[len] < 0) head[len] = n_rem;
    else nxt[tail[len]] = (int16_t)n_rem;
    tail[len] = n_rem++;
  };
  for (int i = 0; i < n; i++) {
    if (i >= 2 && row[i - 2] + 2 == row[i]) continue;  // inside a chain
    int len = 1;
    while (i + 2 * len < n && row[i + 2 * len - 2] + 2 == row[i + 2 * len]) len++;
    const int full = len / HS_TILE_SLOTS * HS_TILE_SLOTS;
    for (int j = 0; j < full; j++) step[out++] = (int16_t)(i + 2 * j);
    if (len > full) push(i + 2 * full, len - full);
  }
  while (out < n) {
    int cap = n - out < HS_TILE_SLOTS ? n - out : HS_TILE_SLOTS;
    while (cap > 0) {
      int len = cap < HS_TILE_SLOTS - 1 ? cap : HS_TILE_SLOTS - 1;
      while (len > 0 && head[len] < 0) len--;
      int take = len;
      if (len == 0) {  // every remainder left is longer than the tile's room: split the shortest
        for (len = cap + 1; head[len] < 0; len++) {}
        take = cap;
      }
      const int r = head[len], first = rem0[r];
      head[len] = nxt[r];
      if (head[len] < 0) tail[len] = -1;
      for (int j = 0; j < take; j++) step[out++] = (int16_t)(first + 2 * j);
      if (len > take) push(first + 2 * take, len - take);
      cap -= take;
    }
  }
  for (; out < n_slots; out++) step[out] = -1;
}

// The launch's sequence: the chain-aligned one where it needs fewer passes than the parity order, else
// the parity order. Returns whether step[] holds the former.
// *passes / *parity_passes: the further FK passes of the sequence kept and of the parity order.
HS_TILE_FN bool limb_tile_plan_rows(const int* row, int n, int n_limbs, int16_t* step, int* passes = nullptr,
                                    int* parity_passes = nullptr) {
  int16_t par[HS_TILE_PLAN_STEPS];
  limb_tile_parity_fill(n, par);
  const int pp = limb_tile_passes(row, n, n_limbs, par);
  int pc = pp;
  if (pp > 0) {  // (nothing to save otherwise: a four-limb model's E0 = 8 takes every request of most tiles)
    limb_tile_chain_fill(row, n, step);
    pc = limb_tile_passes(row, n, n_limbs, step);
  }
  if (parity_passes) *parity_passes = pp;
  if (passes) *passes = pc < pp ? pc : pp;
  if (pc < pp) return true;
  for (int s = 0; s < HS_TILE_SLOTS * limb_tile_count(n); s++) step[s] = par[s];
  return false;
}
// the same from the launch. One longer than a plan holds keeps the parity order (step[] is then not
// written: the caller uses limb_tile_step).
HS_TILE_FN bool limb_tile_plan(const limb_tile_launch& L, int16_t* step, int* passes = nullptr,
                               int* parity_passes = nullptr) {
  if (L.n < 1 || L.n > HS_TILE_PLAN_STEPS || L.h < 1 || L.n_t < 1 || L.k0 < 0 || L.s0 < 0) return false;
  int row[HS_TILE_PLAN_STEPS];
  limb_tile_rows(L, row);
  return limb_tile_plan_rows(row, L.n, L.n_limbs, step, passes, parity_passes);
}

// ---- the tile descriptor ----
// What the TILE kernels take of a launch's slot sequence (a by-value kernel argument, limb_tile_desc_build's
// from the sequence kept: the planner's or the parity order): per tile, every slot's local step and table
// row, and the tile's requests. All of it is the same for every rollout of the launch, so the host forms it
// once and the kernel reads it (limb_step, limb_tile_kd) instead of deriving it per lane and tile. What
// depends on the wavefront's model stays in the kernel: E0 and with it the pass of a request.
constexpr int HS_TILE_DESC_TILES = HS_TILE_PLAN_STEPS / HS_TILE_SLOTS;  // 32

struct alignas(4) limb_tile_slot {
  int16_t step;  // the slot's local step, -1 for an idle slot
  int16_t row;   // limb_tile_row of that step; an idle slot holds the row of the tile's slot 0
};
struct limb_tile_entry {
  limb_tile_slot slot[HS_TILE_SLOTS];
  uint32_t M;     // the requests: bit 2 g slot g's minus row, bit 2 g + 1 its plus row (limb_tile_requests' rule)
  uint32_t nreq;  // their number
  uint64_t req;   // the requests in service order (ascending bit of M), 4 bits each: request r is (req >> 4 r) & 15
};
struct limb_tile_desc {
  int32_t n_tiles;  // limb_tile_count(n)
  int32_t pad_;
  limb_tile_entry tile[HS_TILE_DESC_TILES];
};
static_assert(sizeof(limb_tile_entry) == 48, "a tile's descriptor: 8 slots of 4 bytes, M, nreq and the request list");
static_assert(sizeof(limb_tile_desc) == 8 + 48 * HS_TILE_DESC_TILES && sizeof(limb_tile_desc) <= 1600,
              "the descriptor travels by value: with the kernel's other arguments well under 4 KB");

// whether a descriptor holds the launch: a plan's length, and rows that fit 16 bits
HS_TILE_FN bool limb_tile_desc_ok(int n, int h, int k0, int n_t) {
  return n >= 1 && n <= HS_TILE_PLAN_STEPS && h >= 1 && n_t >= 1 && k0 >= 0 && (int64_t)n_t + h <= 32767;
}

// one tile's entry from its eight slots (step[g], -1 idle) and the launch's steps' rows
HS_TILE_FN void limb_tile_entry_fill(const int* row, const int16_t* slots, limb_tile_entry& e) {
  const int first = slots[0] >= 0 ? row[slots[0]] : 0;
  for (int g = 0; g < HS_TILE_SLOTS; g++) {
    e.slot[g].step = (int16_t)(slots[g] >= 0 ? slots[g] : -1);
    e.slot[g].row = (int16_t)(slots[g] >= 0 ? row[slots[g]] : first);
  }
  e.M = limb_tile_request_mask(row, slots);
  e.nreq = 0;
  e.req = 0;
  for (int bit = 0; bit < 2 * HS_TILE_SLOTS; bit++)
    if ((e.M >> bit) & 1) e.req |= (uint64_t)bit << (4 * e.nreq++);
}

// the descriptor of a sequence step[8 * limb_tile_count(n)] over the launch's rows (limb_tile_rows); the tiles
// past the launch are idle ones: every step -1, every row 0, no request
HS_TILE_FN void limb_tile_desc_fill_rows(const int* row, int n, const int16_t* step, limb_tile_desc& d) {
  const int16_t idle[HS_TILE_SLOTS] = {-1, -1, -1, -1, -1, -1, -1, -1};
  d.n_tiles = limb_tile_count(n);
  d.pad_ = 0;
  for (int t = 0; t < HS_TILE_DESC_TILES; t++)
    limb_tile_entry_fill(row, t < d.n_tiles ? step + HS_TILE_SLOTS * t : idle, d.tile[t]);
}
// the descriptor of a launch's sequence step[8 * limb_tile_count(L.n)] (limb_tile_plan's, limb_tile_chain_fill's
// or limb_tile_parity_fill's). False, and d untouched, where limb_tile_desc_ok says no.
HS_TILE_FN bool limb_tile_desc_fill(const limb_tile_launch& L, const int16_t* step, limb_tile_desc& d) {
  if (!limb_tile_desc_ok(L.n, L.h, L.k0, L.n_t) || L.s0 < 0) return false;
  int row[HS_TILE_PLAN_STEPS];
  limb_tile_rows(L, row);
  limb_tile_desc_fill_rows(row, L.n, step, d);
  return true;
}

// A launch's descriptor under the sequence `mode` chooses, the rows computed once: 0 the parity order, 1 the
// planner's choice (limb_tile_plan), 2 the chain-aligned sequence whatever it saves. *planned: whether the
// sequence is the chain-aligned one. False, and d untouched, for a launch no descriptor holds.
HS_TILE_FN bool limb_tile_desc_build(const limb_tile_launch& L, int mode, limb_tile_desc& d, bool* planned = nullptr) {
  if (planned) *planned = false;
  if (!limb_tile_desc_ok(L.n, L.h, L.k0, L.n_t) || L.s0 < 0) return false;
  int row[HS_TILE_PLAN_STEPS];
  int16_t step[HS_TILE_PLAN_STEPS];
  limb_tile_rows(L, row);
  bool chain = mode == 2;
  if (chain) limb_tile_chain_fill(row, L.n, step);
  else if (mode) chain = limb_tile_plan_rows(row, L.n, L.n_limbs, step);
  else limb_tile_parity_fill(L.n, step);
  limb_tile_desc_fill_rows(row, L.n, step, d);
  if (planned) *planned = chain;
  return true;
}
