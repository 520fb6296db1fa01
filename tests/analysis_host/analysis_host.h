// analysis_host.h -- TEST-ONLY: what the host builds of the terrain analyses (tests/<name>_host/<name>_host.cpp) share around their
// run_* templates: the map of top records, the member table, the poisoned planes and record tables, the tile shapes with their
// dispatch, the record cut and the planes' way out. The run_* templates restate each library call's launch sequence and stay in their
// own files; nothing here knows an analysis. The product never includes this file.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <vector>

#define SMX_D inline
#define SMX_HOSTSIM 1
#include "../../soilmachine_amd/csrc/soil_core.h"
#include "../../soilmachine_amd/csrc/soil_lakes.h"

using namespace smx;

// ---- a map: the top record of every column of a snapshot
struct ah_map {
  int dimx, dimy;
  std::vector<Sec> cells;
};
// columns bottom -> top in cell order (the snapshot layout): a map keeps each column's top record
static ah_map* ah_create(int dimx, int dimy, const uint32_t* count, const uint32_t* type, const double* size, const double* floor) {
  ah_map* m = new ah_map();
  m->dimx = dimx; m->dimy = dimy;
  const size_t n = (size_t)dimx * dimy;
  m->cells.resize(n);
  size_t off = 0;
  for (size_t i = 0; i < n; i++) {
    Sec c; c.size = c.floor = c.sat = 0; c.type = EMPTY; c.prev = NIL;
    if (count[i]) { const size_t t = off + count[i] - 1; c.size = size[t]; c.floor = floor[t]; c.type = type[t]; }
    off += count[i];
    m->cells[i] = c;
  }
  return m;
}

// block b of nb in launch order
static inline uint32_t nth(uint32_t b, uint32_t nb, int descending) { return descending ? nb - 1u - b : b; }
static inline bool lanes_ok(uint32_t lanes) { return lanes == 64 || lanes == 128 || lanes == 256; }

// ---- the member table, as plan_members of soilmx.hip lays it out. A member holds at most as many records as it can have lakes
// (CAP_BLOCKS: the census), as it has cells (CAP_CELLS), or none before the chain has counted its basins (CAP_NONE: spill, through).
enum CapRule { CAP_BLOCKS, CAP_CELLS, CAP_NONE };
struct Members {
  std::vector<LakeMember> tab;
  uint64_t words = 0, nrec = 0, largest = 0;   // the cells of all maps, the records of all maps, the cells of the largest map
};
static Members plan_members(ah_map* const* maps, uint32_t nm, uint32_t cap, CapRule rule) {
  Members pl;
  pl.tab.resize(nm);
  for (uint32_t i = 0; i < nm; i++) {
    LakeMember& m = pl.tab[i];
    m.cells = maps[i]->cells.data(); m.dimx = maps[i]->dimx; m.dimy = maps[i]->dimy; m.pad = 0;
    m.off = (uint32_t)pl.words; m.rec0 = (uint32_t)pl.nrec;
    const uint64_t cells = (uint64_t)m.dimx * m.dimy;
    const uint64_t most = rule == CAP_BLOCKS ? (uint64_t)((m.dimx + 1) / 2) * (uint64_t)((m.dimy + 1) / 2) : rule == CAP_CELLS ? cells : 0u;
    m.cap = (uint32_t)std::min<uint64_t>(cap, most);
    pl.words += cells; pl.nrec += m.cap;
    pl.largest = std::max(pl.largest, cells);
  }
  return pl;
}
// spill and through, the chain's counts back: a record for every basin (plan_basins of soilmx.hip)
static void plan_basins(Members& pl, const uint32_t* counts) {
  pl.nrec = 0;
  for (LakeMember& m : pl.tab) { m.cap = *counts++; m.rec0 = (uint32_t)pl.nrec; pl.nrec += m.cap; }
}

// ---- planes and record tables as the device's: whatever the last call left
static void poison(std::initializer_list<std::vector<uint32_t>*> planes, uint64_t words) {
  for (std::vector<uint32_t>* v : planes) v->assign(words, 0xDEADBEEFu);
}
template <class Acc>
static std::vector<Acc> poisoned_records(uint64_t nrec) {
  std::vector<Acc> acc(nrec ? nrec : 1);
  memset(acc.data(), 0xAB, acc.size() * sizeof(Acc));
  return acc;
}

// ---- the tile shapes: (tile columns, tile rows, slots of the statistics table), and for spill and through the slots of the pass
// table as well. Shape 0 is the kernels' own, shape 2 a tile no dimension is a multiple of.
struct Shape { int tx, ty, slots, pslots; };
static constexpr Shape TILE_SHAPES[4] = {{16, 64, 512, 0}, {8, 8, 256, 0}, {5, 7, 320, 0}, {32, 4, 1024, 0}};
static constexpr Shape PASS_SHAPES[4] = {{16, 64, 512, 1024}, {8, 8, 256, 64}, {5, 7, 320, 40}, {32, 4, 1024, 128}};
template <size_t N>
static const Shape* shape_at(const Shape (&table)[N], int v) { return v < 0 || v >= (int)N ? nullptr : table + v; }

template <const auto& TABLE, size_t V>
struct ShapeAt { static constexpr int TX = TABLE[V].tx, TY = TABLE[V].ty, SLOTS = TABLE[V].slots, PS = TABLE[V].pslots; };
// body(s) for shape `variant` of TABLE, decltype(s)::TX and the others being compile-time constants; false: no such variant
template <const auto& TABLE, size_t V = 0, class Body>
static bool with_shape(int variant, Body&& body) {
  if constexpr (V == sizeof(TABLE) / sizeof(TABLE[0])) return false;
  else {
    if (variant != (int)V) return with_shape<TABLE, V + 1>(variant, body);
    body(ShapeAt<TABLE, V>{});
    return true;
  }
}

// ---- the records of every map: min(count, cap) of them, finish(j, rec) filling rec from entry j of the tables, the first struct_size
// bytes of each to record i * cap + r of out
template <class Rec, class Finish>
static void cut_records(const Members& pl, const uint32_t* counts, uint32_t cap, void* out, size_t struct_size, Finish&& finish) {
  for (size_t i = 0; i < pl.tab.size(); i++) {
    const uint32_t w = std::min({counts[i], pl.tab[i].cap, cap});
    for (uint32_t r = 0; r < w; r++) {
      Rec rec;
      finish((size_t)pl.tab[i].rec0 + r, rec);
      memcpy(static_cast<char*>(out) + (i * cap + r) * struct_size, &rec, std::min(struct_size, sizeof(rec)));
    }
  }
}
// a plane of all maps, one after the other, to the caller (NULL = skip)
template <class T>
static void copy_plane(T* to, const T* from, uint64_t words) { if (to) memcpy(to, from, words * sizeof(T)); }
