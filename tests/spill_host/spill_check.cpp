// spill_check -- a stand-alone run of the spill bodies for the sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o spill_check spill_check.cpp && ./spill_check
// Without arguments: random heights, random heights under a Bernoulli(0.2) wet mask, a plateau and a sawtooth at 33 x 47 and 96 x 80,
// and three maps in one call: every tile shape, 64 and 256 lanes, the four launch orders and relax sweeps of 1, 3 and all workgroups must
// give the same records and the same filled plane as the kernels' own shape in ascending order at full width, every fill level lies at or above its pour height, and filled(c) is
// max(h(c), the level of c's basin) by the ordered image.
// With arguments: each names a dump written by tests/test_spill_host.py -- an input of tests/spill_ref.py with the restatement's
// result: the columns' top records exactly as the snapshot holds them, then the count, the records and the filled plane, all compared
// bit by bit. Every tile shape, 64 and 256 lanes, workgroups and lanes first to last and last to first, relax sweeps of 1, 3 and all
// workgroups. Little-endian words:
//   u32 magic 0x4C495053, i32 dimx, i32 dimy, u32 nsec, u32 count[cells], u32 type[nsec], f64 size[nsec], f64 floor[nsec],
//   u32 nbasins, 64-byte records[nbasins], f64 filled[cells]
// Exit status 0 = all equal.
#include "spill_host.cpp"
#include "../analysis_host/analysis_check.h"

struct Result { std::vector<uint32_t> nb; std::vector<SpillRec> recs; std::vector<double> filled; uint32_t sweeps = 0, batches = 0; };

constexpr uint32_t FULL = 0xFFFFFFFFu;   // relax_blocks: a lane per cell, no stride
// (the capped sweeps on the kernels' own tile shape alone: no strided body works on tiles)
static std::vector<uint32_t> widths(int v) { return v == 0 ? std::vector<uint32_t>{FULL, 1u, 3u} : std::vector<uint32_t>{FULL}; }
static bool run(const std::vector<dh_map*>& maps, int v, uint32_t lanes, int order, uint32_t relax_blocks, uint32_t cap, Result& r) {
  size_t words = 0;
  for (const dh_map* m : maps) words += m->cells.size();
  r.nb.assign(maps.size(), 0); r.recs.assign(maps.size() * (size_t)cap + 1, SpillRec()); r.filled.assign(words, 0.0);
  memset(r.recs.data(), 0, r.recs.size() * sizeof(SpillRec));
  return sh_spill(maps.data(), (uint32_t)maps.size(), v, lanes, order, relax_blocks, cap, r.recs.data(), sizeof(SpillRec), r.nb.data(), r.filled.data(), &r.sweeps, &r.batches) == 0;
}

static int check(const char* name, const std::vector<dh_map*>& maps) {
  uint32_t cap = 0;
  for (const dh_map* m : maps) cap = std::max<uint32_t>(cap, (uint32_t)m->cells.size());
  Result want;
  int bad = run(maps, 0, 256, 0, FULL, cap, want) ? 0 : 1;
  size_t at = 0;
  for (size_t i = 0; i < maps.size() && !bad; i++) {
    const dh_map* m = maps[i];
    for (uint32_t k = 0; k < want.nb[i]; k++) {
      const SpillRec& s = want.recs[i * (size_t)cap + k];
      if (lake_key(s.fill_height) < lake_key(s.pour_height) || s.first_cell >= m->cells.size() || s.pour_cell >= m->cells.size()) bad++;
    }
    for (size_t c = 0; c < m->cells.size(); c++)
      if (lake_key(want.filled[at + c]) < lake_key(drain_height(m->cells[c]))) bad++;
    at += m->cells.size();
  }
  if (bad) printf("FAIL %s: the kernels' own shape\n", name);
  for (int v = 0; v < sh_variants(); v++)
    for (uint32_t lanes : {64u, 256u})
      for (int order = 0; order < 4; order++)
        for (uint32_t blocks : widths(v)) {
          Result got;
          const bool same = run(maps, v, lanes, order, blocks, cap, got) && got.nb == want.nb &&
                            memcmp(got.recs.data(), want.recs.data(), want.recs.size() * sizeof(SpillRec)) == 0 &&
                            memcmp(got.filled.data(), want.filled.data(), want.filled.size() * 8) == 0;
          if (!same) { printf("FAIL %s variant %d lanes %u order %d relax_blocks %u\n", name, v, lanes, order, blocks); bad++; }
        }
  printf("%-10s %zu map(s), %5u basins in the first, %3u sweeps  %s\n", name, maps.size(), want.nb.empty() ? 0u : want.nb[0], want.sweeps, bad ? "FAILED" : "ok");
  return bad;
}

static int check_dump(const char* path) {
  Columns in;
  uint32_t nb = 0;
  std::vector<double> filled;
  std::vector<SpillRec> recs;
  if (!read_dump(path, 0x4C495053u, in, [&](FILE* f) { return fread(&nb, 4, 1, f) == 1 && nb <= in.cells && take(f, recs, nb) && take(f, filled, in.cells); })) return 1;
  const size_t n = in.cells;
  std::vector<dh_map*> maps{in.map()};
  int bad = 0;
  for (int v = 0; v < sh_variants(); v++)
    for (uint32_t lanes : {64u, 256u})
      for (int order : {0, 3})
        for (uint32_t blocks : widths(v)) {
          Result got;
          const bool same = run(maps, v, lanes, order, blocks, nb + 2u, got) && got.nb[0] == nb &&
                            (nb == 0 || memcmp(got.recs.data(), recs.data(), (size_t)nb * sizeof(SpillRec)) == 0) && memcmp(got.filled.data(), filled.data(), n * 8) == 0;
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
