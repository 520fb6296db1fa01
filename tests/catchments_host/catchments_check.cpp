// catchments_check -- a stand-alone run of the catchment bodies for the sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o catchments_check catchments_check.cpp && ./catchments_check
// Without arguments: a ramp, a plateau, random heights and random heights under a Bernoulli(0.2) wet mask at 33 x 47 and 96 x 80, and
// three maps in one call with one list, every tile shape, 64 and 256 lanes, the four launch orders, with three lists each -- one
// cell, every 7th cell, every cell -- and 0, 1 and 64 bins, against one plain walk per cell down the receivers of the drainage host
// build (the four planes per cell, the tables, the records field by field, area summed by a walk down the gauges from every gauge).
// With arguments: each names a dump written by tests/test_catchments_host.py -- the hand-built map, the spiral with its line of
// gauges or another input of tests/drainage_ref.py with the restatement's result: the columns' top records exactly as the snapshot
// holds them, then the list, the four planes, the table and the records, all compared bit by bit. Every tile shape, 64 and 256 lanes,
// workgroups and lanes first to last and last to first. Little-endian words:
//   u32 magic 0x48544143, i32 dimx, i32 dimy, u32 nsec, u32 count[cells], u32 type[nsec], f64 size[nsec], f64 floor[nsec],
//   u32 n, u32 nbins, f64 bin_height, u32 list[n], u32 gauge[cells], u32 straight[cells], u32 diagonal[cells], f64 drop[cells],
//   u32 hist[n * nbins], 64-byte records[n]
// Exit status 0 = all equal.
#include "catchments_host.cpp"
#include "../analysis_host/analysis_check.h"

struct Want { std::vector<uint32_t> gauge, st, dg, hist; std::vector<double> drop; std::vector<CatchRec> recs; };

// one walk per cell down the receivers to the first gauge, sink or wet cell; the records summed in cell order
static Want plain(const Input& in, dh_map* h, const std::vector<uint32_t>& list, uint32_t nbins, double bin_height) {
  const size_t n = in.h.size();
  const uint32_t dy = (uint32_t)in.dy, ng = (uint32_t)list.size();
  uint32_t nb = 0;
  std::vector<uint32_t> recv(n), lab(n), pos(n, CATCH_NONE);
  std::vector<BasinRec> brec(n + 1);
  if (dh_drainage(&h, 1, 0, 256, 0, (uint32_t)n, brec.data(), &nb, recv.data(), lab.data(), nullptr) != 0) exit(2);
  for (uint32_t i = 0; i < ng; i++) pos[list[i]] = i;
  auto height = [&](size_t c) { return in.wet[c] ? in.h[c] + 0.5 : in.h[c]; };
  Want w;
  w.gauge.assign(n, CATCH_NONE); w.st.assign(n, 0u); w.dg.assign(n, 0u); w.drop.assign(n, 0.0); w.hist.assign((size_t)ng * nbins, 0u);
  w.recs.resize(ng);
  memset(w.recs.data(), 0, ng * sizeof(CatchRec));
  for (uint32_t i = 0; i < ng; i++) {
    CatchRec& r = w.recs[i];
    const uint32_t g = list[i];
    r.cell = g; r.basin = lab[g]; r.farthest_cell = g;
    r.downstream = CATCH_NONE;
    if (recv[g] == DRAIN_NONE) r.flags = in.wet[g] ? CATCH_F_WET : CATCH_F_SINK;
  }
  for (uint32_t c = 0; c < n; c++) {
    uint32_t e = c, s = 0, d = 0;
    while (pos[e] == CATCH_NONE && recv[e] != DRAIN_NONE) {
      const uint32_t r = recv[e];
      if (r / dy != e / dy && r % dy != e % dy) d++; else s++;
      e = r;
    }
    w.gauge[c] = pos[e]; w.st[c] = s; w.dg[c] = d;
    if (e != c) w.drop[c] = height(c) - height(e);
    if (pos[e] == CATCH_NONE) continue;
    CatchRec& r = w.recs[pos[e]];
    r.cells++; r.straight_sum += s; r.diagonal_sum += d;
    if (s + d > r.steps_max) { r.steps_max = s + d; r.farthest_cell = c; }   // (ascending c: of equal steps the first stays)
    if (w.drop[c] > r.drop_max) r.drop_max = w.drop[c];                        // (finite and not negative in these inputs)
    r.drop_sum_q40 += (uint64_t)floor(w.drop[c] * 1099511627776.0);
    if (nbins) {
      const double q = w.drop[c] / bin_height;
      w.hist[(size_t)pos[e] * nbins + (q < nbins ? (uint32_t)q : nbins - 1u)]++;
    }
  }
  for (uint32_t i = 0; i < ng; i++) {
    const uint32_t g = list[i];
    if (recv[g] != DRAIN_NONE) w.recs[i].downstream = w.gauge[recv[g]];
  }
  for (uint32_t i = 0; i < ng; i++)   // every gauge adds its own cells to itself and to every gauge below it
    for (uint32_t j = i; j != CATCH_NONE; j = w.recs[j].downstream) w.recs[j].area += w.recs[i].cells;
  return w;
}

static bool equal_to(const Want& w, size_t cells, const uint32_t* g, const uint32_t* st, const uint32_t* dg, const double* dr, const uint32_t* hist, const CatchRec* out) {
  return std::equal(w.gauge.begin(), w.gauge.end(), g) && std::equal(w.st.begin(), w.st.end(), st) && std::equal(w.dg.begin(), w.dg.end(), dg) && same_bits(w.drop, dr) &&
         w.gauge.size() == cells && std::equal(w.hist.begin(), w.hist.end(), hist) && memcmp(out, w.recs.data(), w.recs.size() * sizeof(CatchRec)) == 0;
}

static int check(const char* name, const std::vector<Input>& ins) {
  std::vector<dh_map*> maps;
  size_t words = 0, least = ~(size_t)0;
  for (const Input& in : ins) { maps.push_back(host_map(in)); words += in.h.size(); least = std::min(least, in.h.size()); }
  const uint32_t nm = (uint32_t)ins.size();
  int bad = 0;
  std::vector<std::vector<uint32_t>> lists(3);
  lists[0] = {(uint32_t)(least / 2)};
  for (uint32_t c = 0; c < least; c += 7) lists[1].push_back((uint32_t)(least - 1 - c));   // (descending: positions are not cell order)
  for (uint32_t c = 0; c < least; c++) lists[2].push_back(c);
  size_t gauges = 0;
  for (size_t li = 0; li < lists.size(); li++) {
    const std::vector<uint32_t>& list = lists[li];
    const uint32_t n = (uint32_t)list.size(), nbins = li == 0 ? 1u : li == 1 ? 64u : 0u;
    const double bh = 0.0078125;   // (2^-7: the heights are multiples of 2^-10, many drops lie exactly on an edge)
    std::vector<Want> wants;
    for (uint32_t i = 0; i < nm; i++) wants.push_back(plain(ins[i], maps[i], list, nbins, bh));
    gauges += n;
    for (int v = 0; v < dh_variants(); v++)
      for (uint32_t lanes : {64u, 256u})
        for (int order : {0, 1, 2, 3}) {
          std::vector<uint32_t> g(words), st(words), dg(words), hist((size_t)nm * n * nbins + 1u, 0xDEADBEEFu);
          std::vector<double> dr(words);
          std::vector<CatchRec> out((size_t)nm * n + 1u);
          memset(out.data(), 0xEE, out.size() * sizeof(CatchRec));
          if (ch_catchments(maps.data(), nm, v, lanes, order, list.data(), n, out.data(), sizeof(CatchRec), nbins ? hist.data() : nullptr, nbins, bh, g.data(), st.data(),
                            dg.data(), dr.data(), nullptr) != 0) { bad++; continue; }
          bool ok = hist.back() == 0xDEADBEEFu && out.back().cell == 0xEEEEEEEEu;   // (nothing behind what was asked for)
          size_t at = 0;
          for (uint32_t i = 0; i < nm && ok; i++) {
            ok = equal_to(wants[i], ins[i].h.size(), g.data() + at, st.data() + at, dg.data() + at, dr.data() + at, hist.data() + (size_t)i * n * nbins, out.data() + (size_t)i * n);
            at += ins[i].h.size();
          }
          if (!ok) { printf("FAIL %s list %zu variant %d lanes %u order %d\n", name, li, v, lanes, order); bad++; }
        }
  }
  for (dh_map* m : maps) dh_destroy(m);
  printf("%-10s %zu map(s), %6zu gauges in three lists  %s\n", name, ins.size(), gauges, bad ? "FAILED" : "ok");
  return bad;
}

static int check_dump(const char* path) {
  Columns in;
  uint32_t head[2] = {0, 0};
  double bh = 0.0;
  std::vector<uint32_t> list, g, st, dg, hist;
  std::vector<double> dr;
  std::vector<CatchRec> recs;
  if (!read_dump(path, 0x48544143u, in, [&](FILE* f) {
        const size_t n = in.cells;
        return fread(head, 4, 2, f) == 2 && head[0] >= 1 && head[0] <= n && head[1] <= CATCH_MAX_BINS && fread(&bh, 8, 1, f) == 1 && take(f, list, head[0]) && take(f, g, n) &&
               take(f, st, n) && take(f, dg, n) && take(f, dr, n) && take(f, hist, (size_t)head[0] * head[1]) && take(f, recs, head[0]);
      })) return 1;
  const size_t n = in.cells;
  const uint32_t ng = head[0], nbins = head[1];
  for (uint32_t c : list)
    if (c >= n) { printf("FAIL %s lists a cell outside the map\n", path); return 1; }
  dh_map* h = in.map();
  int bad = 0;
  for (int v = 0; v < dh_variants(); v++)
    for (uint32_t lanes : {64u, 256u})
      for (int order : {0, 3}) {
        std::vector<uint32_t> a(n), b(n), c(n), t((size_t)ng * nbins + 1u);
        std::vector<double> q(n);
        std::vector<CatchRec> out(ng);
        const bool same = ch_catchments(&h, 1, v, lanes, order, list.data(), ng, out.data(), sizeof(CatchRec), nbins ? t.data() : nullptr, nbins, bh, a.data(), b.data(), c.data(),
                                        q.data(), nullptr) == 0 &&
                          a == g && b == st && c == dg && same_bits(dr, q.data()) && std::equal(hist.begin(), hist.end(), t.begin()) &&
                          memcmp(out.data(), recs.data(), (size_t)ng * sizeof(CatchRec)) == 0;
        if (!same) { printf("FAIL %s variant %d lanes %u order %d\n", path, v, lanes, order); bad++; }
      }
  dh_destroy(h);
  printf("%-36s %4ux%-4u %6u gauges, %2u bins  %s\n", file_name(path), in.dimx, in.dimy, ng, nbins, bad ? "FAILED" : "ok");
  return bad;
}

int main(int argc, char** argv) {
  return check_main(argc, argv, check_dump, {"ramp", "plateau", "random", "lakes"}, {{"lakes", 33, 47}, {"random", 70, 1}, {"random", 1, 70}},
                    [](const char* name, const std::vector<MapSpec>& specs) { return check(name, make_all(specs)); });
}
