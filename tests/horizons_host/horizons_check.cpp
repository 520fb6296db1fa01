// horizons_check -- a stand-alone run of the horizon bodies for the sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o horizons_check horizons_check.cpp && ./horizons_check
// Without arguments: a cone, a ramp, a plateau, random heights and random heights under a Bernoulli(0.2) wet mask at 33 x 47 and
// 96 x 80, and three maps in one call, every tile shape, 64 and 256 lanes with two of the four launch orders each, with reach 0 and 5, all sixteen
// directions and one mask of three, and three suns, against one plain walk per cell and direction to the map's edge (the five planes
// per cell, the sun counts, the records field by field).
// With arguments: each names a dump written by tests/test_horizons_host.py -- an input of tests/horizons_ref.py with the
// restatement's result: the columns' top records exactly as the snapshot holds them, then the call and what it has to give, all
// compared bit by bit. Every tile shape, 64 and 256 lanes, workgroups and lanes first to last and last to first. Little-endian words:
//   u32 magic 0x5A524F48, i32 dimx, i32 dimy, u32 nsec, u32 count[cells], u32 type[nsec], f64 size[nsec], f64 floor[nsec],
//   u32 mask, u32 reach, u32 nsuns, u32 0, 16-byte suns[nsuns], f64 slope[nd * cells], u32 step[nd * cells], f64 sky[cells],
//   u32 open[cells], u32 lit[cells], u32 lit_cells[nsuns], 64-byte records[nd]
// Exit status 0 = all equal.
#include "horizons_host.cpp"
#include "../analysis_host/analysis_check.h"

struct Want { std::vector<double> S, sky; std::vector<uint32_t> K, open, lit, counts; std::vector<HorizonRec> recs; };

// one walk per cell and direction, every step; the records folded in cell order
static Want plain(const Input& in, uint32_t mask, uint32_t reach, const std::vector<HorizonSun>& suns) {
  const size_t n = in.h.size();
  const int dx = in.dx, dy = in.dy;
  const uint32_t nd = horizon_count(mask);
  auto height = [&](size_t c) { return in.wet[c] ? in.h[c] + 0.5 : in.h[c]; };
  Want w;
  w.S.assign(nd * n, 0.0); w.K.assign(nd * n, 0u); w.sky.assign(n, 0.0); w.open.assign(n, 0u); w.lit.assign(n, 0u); w.counts.assign(suns.size(), 0u);
  w.recs.resize(nd);
  memset(w.recs.data(), 0, nd * sizeof(HorizonRec));
  for (uint32_t j = 0; j < nd; j++) {
    const uint32_t d = horizon_nth(mask, j);
    int ux, uy;
    horizon_dir(d, ux, uy);
    HorizonRec& r = w.recs[j];
    r.direction = d; r.ux = (int16_t)ux; r.uy = (int16_t)uy; r.step_max_cell = 0xFFFFFFFFu;
    for (size_t c = 0; c < n; c++) {
      const int x = (int)(c / dy), y = (int)(c % dy);
      double best = 0.0;
      uint32_t bk = 0;
      for (uint32_t k = 1; !reach || k <= reach; k++) {
        const int px = x + (int)k * ux, py = y + (int)k * uy;
        if (px < 0 || px >= dx || py < 0 || py >= dy) break;
        const double s = (height((size_t)px * dy + py) - height(c)) / ((double)k * horizon_len(d));
        if (s > best) { best = s; bk = k; }
      }
      w.S[j * n + c] = best; w.K[j * n + c] = bk;
      if (!bk) continue;
      r.bounded++; r.step_sum += bk;
      if (bk > r.step_max) { r.step_max = bk; r.step_max_cell = (uint32_t)c; }   // (ascending c: of equal steps the first stays)
      if (best > r.slope_max) r.slope_max = best;
    }
  }
  for (size_t c = 0; c < n; c++) {
    double sum = 0.0;
    for (uint32_t j = 0; j < nd; j++) {
      const double s = w.S[j * n + c];
      sum = sum + 1.0 / (1.0 + s * s);
      if (!w.K[j * n + c]) w.open[c] |= 1u << horizon_nth(mask, j);
    }
    w.sky[c] = sum / (double)nd;
    for (size_t i = 0; i < suns.size(); i++) {
      const uint32_t j = horizon_count(mask & ((1u << suns[i].direction) - 1u));
      if (!(w.S[j * n + c] > suns[i].tangent)) { w.lit[c]++; w.counts[i]++; }
    }
  }
  return w;
}

static int check(const char* name, const std::vector<Input>& ins) {
  std::vector<dh_map*> maps;
  size_t words = 0;
  for (const Input& in : ins) { maps.push_back(host_map(in)); words += in.h.size(); }
  const uint32_t nm = (uint32_t)ins.size();
  int bad = 0;
  size_t runs = 0;
  for (uint32_t mask : {0xFFFFu, 0x0212u})
    for (uint32_t reach : {0u, 5u}) {
      const uint32_t nd = horizon_count(mask);
      const std::vector<HorizonSun> suns = {{horizon_nth(mask, 0), 0u, 0.0}, {horizon_nth(mask, nd / 2), 0u, 0.0078125}, {horizon_nth(mask, nd - 1), 0u, 1.0e6}};
      const uint32_t ns = (uint32_t)suns.size();
      std::vector<Want> wants;
      for (const Input& in : ins) wants.push_back(plain(in, mask, reach, suns));
      for (int v = 0; v < hz_variants(); v++)
        for (uint32_t lanes : {64u, 256u})
          for (int order : {(int)(lanes == 64u), 2 + (int)(lanes != 64u)}) {
            std::vector<double> S((size_t)nd * words), sky(words);
            std::vector<uint32_t> K((size_t)nd * words), open(words), lit(words), counts((size_t)nm * ns + 1u, 0xDEADBEEFu);
            std::vector<HorizonRec> out((size_t)nm * nd + 1u);
            memset(out.data(), 0xEE, out.size() * sizeof(HorizonRec));
            runs++;
            if (hz_horizons(maps.data(), nm, v, lanes, order, mask, reach, out.data(), sizeof(HorizonRec), suns.data(), ns, counts.data(), S.data(), K.data(), sky.data(),
                            open.data(), lit.data(), nullptr) != 0) { bad++; continue; }
            bool ok = counts.back() == 0xDEADBEEFu && out.back().direction == 0xEEEEEEEEu;   // (nothing behind what was asked for)
            size_t at = 0;
            for (uint32_t i = 0; i < nm && ok; i++) {
              const Want& w = wants[i];
              const size_t n = ins[i].h.size();
              for (uint32_t j = 0; j < nd && ok; j++)
                ok = memcmp(w.S.data() + j * n, S.data() + j * words + at, n * 8) == 0 && memcmp(w.K.data() + j * n, K.data() + j * words + at, n * 4) == 0;
              ok = ok && same_bits(w.sky, sky.data() + at) && std::equal(w.open.begin(), w.open.end(), open.begin() + at) && std::equal(w.lit.begin(), w.lit.end(), lit.begin() + at) &&
                   std::equal(w.counts.begin(), w.counts.end(), counts.begin() + (size_t)i * ns) && memcmp(out.data() + (size_t)i * nd, w.recs.data(), nd * sizeof(HorizonRec)) == 0;
              at += n;
            }
            if (!ok) { printf("FAIL %s mask %04x reach %u variant %d lanes %u order %d\n", name, mask, reach, v, lanes, order); bad++; }
          }
    }
  for (dh_map* m : maps) dh_destroy(m);
  printf("%-10s %zu map(s), %4zu runs  %s\n", name, ins.size(), runs, bad ? "FAILED" : "ok");
  return bad;
}

static int check_dump(const char* path) {
  Columns in;
  uint32_t head[4] = {0, 0, 0, 0};
  std::vector<HorizonSun> suns;
  std::vector<double> S, sky;
  std::vector<uint32_t> K, open, lit, counts;
  std::vector<HorizonRec> recs;
  uint32_t nd = 0;
  if (!read_dump(path, 0x5A524F48u, in, [&](FILE* f) {
        const size_t n = in.cells;
        if (fread(head, 4, 4, f) != 4 || head[0] == 0u || (head[0] >> HORIZON_DIRS) || head[2] > HORIZON_MAX_SUNS) return false;
        nd = horizon_count(head[0]);
        return take(f, suns, head[2]) && take(f, S, nd * n) && take(f, K, nd * n) && take(f, sky, n) && take(f, open, n) && take(f, lit, n) && take(f, counts, head[2]) &&
               take(f, recs, nd);
      })) return 1;
  const size_t n = in.cells;
  const uint32_t mask = head[0], reach = head[1], ns = head[2];
  dh_map* h = in.map();
  int bad = 0;
  for (int v = 0; v < hz_variants(); v++)
    for (uint32_t lanes : {64u, 256u})
      for (int order : {0, 3}) {
        std::vector<double> a((size_t)nd * n), b(n);
        std::vector<uint32_t> k((size_t)nd * n), o(n), l(n), cn(ns + 1u);
        std::vector<HorizonRec> out(nd);
        const bool same = hz_horizons(&h, 1, v, lanes, order, mask, reach, out.data(), sizeof(HorizonRec), ns ? suns.data() : nullptr, ns, ns ? cn.data() : nullptr, a.data(),
                                      k.data(), b.data(), o.data(), ns ? l.data() : nullptr, nullptr) == 0 &&
                          same_bits(S, a.data()) && k == K && same_bits(sky, b.data()) && o == open && (!ns || l == lit) && std::equal(counts.begin(), counts.end(), cn.begin()) &&
                          memcmp(out.data(), recs.data(), (size_t)nd * sizeof(HorizonRec)) == 0;
        if (!same) { printf("FAIL %s variant %d lanes %u order %d\n", path, v, lanes, order); bad++; }
      }
  dh_destroy(h);
  printf("%-36s %4ux%-4u mask %04x reach %u, %u suns  %s\n", file_name(path), in.dimx, in.dimy, mask, reach, ns, bad ? "FAILED" : "ok");
  return bad;
}

int main(int argc, char** argv) {
  return check_main(argc, argv, check_dump, {"cone", "ramp", "plateau", "random", "lakes"}, {{"lakes", 33, 47}, {"random", 70, 1}, {"random", 1, 70}},
                    [](const char* name, const std::vector<MapSpec>& specs) { return check(name, make_all(specs)); });
}
