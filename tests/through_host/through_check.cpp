// through_check -- a stand-alone run of the through-drainage bodies for the sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o through_check through_check.cpp && ./through_check
// Without arguments: random heights, random heights under a Bernoulli(0.2) wet mask, a plateau and a sawtooth at 33 x 47 and 96 x 80,
// and three maps in one call: every tile shape, 64 and 256 lanes, the four launch orders and sweeps of 1, 3 and all workgroups must give
// the same records and the same planes as the kernels' own shape in ascending order at full width; hops strictly falls along down, the roots' through_cells sum to the map and
// no through_area is 0.
// With arguments: each names a dump written by tests/test_through_host.py -- an input of tests/through_ref.py with the restatement's
// result: the columns' top records exactly as the snapshot holds them, then the count, the records and the two planes, all compared
// bit by bit. Every tile shape, 64 and 256 lanes, workgroups and lanes first to last and last to first, sweeps of 1, 3 and all
// workgroups. Little-endian words:
//   u32 magic 0x55524854, i32 dimx, i32 dimy, u32 nsec, u32 count[cells], u32 type[nsec], f64 size[nsec], f64 floor[nsec],
//   u32 nbasins, 64-byte records[nbasins], u32 through_area[cells], u32 outlets[cells]
// Exit status 0 = all equal.
#include "through_host.cpp"
#include "../analysis_host/analysis_check.h"

struct Result { std::vector<uint32_t> nb, area, outlets; std::vector<ThroughRec> recs; uint32_t sweeps[3] = {0, 0, 0}; };

constexpr uint32_t FULL = 0xFFFFFFFFu;   // relax_blocks: a lane per cell, no stride
// (the capped sweeps on the kernels' own tile shape alone: no strided body works on tiles)
static std::vector<uint32_t> widths(int v) { return v == 0 ? std::vector<uint32_t>{FULL, 1u, 3u} : std::vector<uint32_t>{FULL}; }
static bool run(const std::vector<dh_map*>& maps, int v, uint32_t lanes, int order, uint32_t relax_blocks, uint32_t cap, Result& r) {
  size_t words = 0;
  for (const dh_map* m : maps) words += m->cells.size();
  r.nb.assign(maps.size(), 0); r.recs.assign(maps.size() * (size_t)cap + 1, ThroughRec()); r.area.assign(words, 0u); r.outlets.assign(words, 0u);
  memset(r.recs.data(), 0, r.recs.size() * sizeof(ThroughRec));
  return th_through(maps.data(), (uint32_t)maps.size(), v, lanes, order, relax_blocks, cap, r.recs.data(), sizeof(ThroughRec), r.nb.data(), r.area.data(), r.outlets.data(), r.sweeps) == 0;
}

static int check(const char* name, const std::vector<dh_map*>& maps) {
  uint32_t cap = 0;
  for (const dh_map* m : maps) cap = std::max<uint32_t>(cap, (uint32_t)m->cells.size());
  Result want;
  int bad = run(maps, 0, 256, 0, FULL, cap, want) ? 0 : 1;
  size_t at = 0;
  for (size_t i = 0; i < maps.size() && !bad; i++) {
    const dh_map* m = maps[i];
    const ThroughRec* rec = want.recs.data() + i * (size_t)cap;
    uint64_t roots = 0;
    for (uint32_t k = 0; k < want.nb[i]; k++) {
      const ThroughRec& s = rec[k];
      if (s.first_cell >= m->cells.size() || s.exit_cell >= m->cells.size() || s.hops == 0u || s.hops > want.nb[i]) { bad++; continue; }
      if (s.down == THROUGH_NONE) { roots += s.through_cells; if (s.hops != 1u || !(s.flags & THROUGH_F_OFFMAP)) bad++; continue; }
      const ThroughRec* d = std::lower_bound(rec, rec + want.nb[i], s.down, [](const ThroughRec& a, uint32_t f) { return a.first_cell < f; });
      if (d == rec + want.nb[i] || d->first_cell != s.down || d->hops + 1u != s.hops || lake_key(d->fill_height) > lake_key(s.fill_height)) bad++;
    }
    if (roots != m->cells.size()) bad++;
    for (size_t c = 0; c < m->cells.size(); c++)
      if (want.area[at + c] == 0u || want.outlets[at + c] >= want.nb[i]) bad++;
    at += m->cells.size();
  }
  if (bad) printf("FAIL %s: the kernels' own shape\n", name);
  for (int v = 0; v < th_variants(); v++)
    for (uint32_t lanes : {64u, 256u})
      for (int order = 0; order < 4; order++)
        for (uint32_t blocks : widths(v)) {
          Result got;
          const bool same = run(maps, v, lanes, order, blocks, cap, got) && got.nb == want.nb &&
                            memcmp(got.recs.data(), want.recs.data(), want.recs.size() * sizeof(ThroughRec)) == 0 && got.area == want.area && got.outlets == want.outlets;
          if (!same) { printf("FAIL %s variant %d lanes %u order %d relax_blocks %u\n", name, v, lanes, order, blocks); bad++; }
        }
  printf("%-10s %zu map(s), %5u basins in the first, %3u + %3u sweeps  %s\n", name, maps.size(), want.nb.empty() ? 0u : want.nb[0], want.sweeps[0], want.sweeps[1],
         bad ? "FAILED" : "ok");
  return bad;
}

static int check_dump(const char* path) {
  Columns in;
  uint32_t nb = 0;
  std::vector<uint32_t> area, outlets;
  std::vector<ThroughRec> recs;
  if (!read_dump(path, 0x55524854u, in, [&](FILE* f) {
        return fread(&nb, 4, 1, f) == 1 && nb <= in.cells && take(f, recs, nb) && take(f, area, in.cells) && take(f, outlets, in.cells);
      })) return 1;
  std::vector<dh_map*> maps{in.map()};
  int bad = 0;
  for (int v = 0; v < th_variants(); v++)
    for (uint32_t lanes : {64u, 256u})
      for (int order : {0, 3})
        for (uint32_t blocks : widths(v)) {
          Result got;
          const bool same = run(maps, v, lanes, order, blocks, nb + 2u, got) && got.nb[0] == nb &&
                            (nb == 0 || memcmp(got.recs.data(), recs.data(), (size_t)nb * sizeof(ThroughRec)) == 0) && got.area == area && got.outlets == outlets;
          if (!same) { printf("FAIL %s variant %d lanes %u order %d relax_blocks %u: %u basins, expected %u\n", path, v, lanes, order, blocks, got.nb[0], nb); bad++; }
        }
  dh_destroy(maps[0]);
  printf("%-32s %4ux%-4u %6u basins  %s\n", file_name(path), in.dimx, in.dimy, nb, bad ? "FAILED" : "ok");
  return bad;
}

int main(int argc, char** argv) {
  return check_main(argc, argv, check_dump, {"random", "lakes", "plateau", "sawtooth"}, {{"lakes", 33, 47}, {"sawtooth", 70, 1}, {"random", 1, 70}},
                    [](const char* name, const std::vector<MapSpec>& specs) { return check_columns(name, specs, check); });
}
