// hillslopes_check -- a stand-alone run of the hillslope bodies for the sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o hillslopes_check hillslopes_check.cpp && ./hillslopes_check
// Without arguments: a cone, a ramp, a plateau, random heights and random heights under a Bernoulli(0.2) wet mask at 33 x 47 and
// 96 x 80, and three maps in one call, thresholds 1, 3 and 40, every tile shape, 64 and 256 lanes, the four launch orders, against a
// plain walk down the receivers of the drainage host build over the segments plane of the streams host build (the five planes per
// cell; the records field by field), with caps above and below the count.
// With arguments: each names a dump written by tests/test_hillslopes_host.py -- an input of tests/drainage_ref.py or the hand-built
// network with the restatement's result for one threshold: the columns' top records exactly as the snapshot holds them, then the
// count, the five planes and the records, all compared bit by bit. Every tile shape, 64 and 256 lanes, workgroups and lanes first to
// last and last to first. Little-endian words:
//   u32 magic 0x4C4C4948, i32 dimx, i32 dimy, u32 nsec, u32 count[cells], u32 type[nsec], f64 size[nsec], f64 floor[nsec],
//   u32 threshold, u32 nsegments, u32 entry[cells], u32 hillslope[cells], u32 straight[cells], u32 diagonal[cells], f64 hand[cells],
//   64-byte records[nsegments]
// Exit status 0 = all equal.
#include "hillslopes_host.cpp"
#include "../analysis_host/analysis_check.h"

struct Want { std::vector<uint32_t> entry, hill, st, dg; std::vector<double> hand; std::vector<HillRec> recs; };

// one walk per cell down the receivers, the figures of a record summed in cell order
static Want plain(const Input& in, dh_map* h, uint32_t threshold) {
  const size_t n = in.h.size();
  const uint32_t dy = (uint32_t)in.dy;
  uint32_t nb = 0, ns = 0;
  std::vector<uint32_t> recv(n), seg(n);
  std::vector<StreamRec> srec(n + 1);
  if (dh_drainage(&h, 1, 0, 256, 0, 0, nullptr, &nb, recv.data(), nullptr, nullptr) != 0) exit(2);
  if (sh_streams(&h, 1, 0, 256, 0, threshold, (uint32_t)n, srec.data(), &ns, nullptr, seg.data(), nullptr, nullptr) != 0) exit(2);
  auto height = [&](size_t c) { return in.wet[c] ? in.h[c] + 0.5 : in.h[c]; };
  Want w;
  w.entry.assign(n, HILL_NONE); w.hill.assign(n, HILL_NONE); w.st.assign(n, 0u); w.dg.assign(n, 0u); w.hand.assign(n, 0.0);
  w.recs.resize(ns);
  for (uint32_t k = 0; k < ns; k++) { memset(&w.recs[k], 0, sizeof(HillRec)); w.recs[k].first_cell = srec[k].first_cell; w.recs[k].farthest_cell = HILL_NONE; }
  for (uint32_t c = 0; c < n; c++) {
    if (in.wet[c]) continue;
    uint32_t e = c, s = 0, d = 0;
    while (seg[e] == STREAM_OFF && recv[e] != DRAIN_NONE) {
      const uint32_t r = recv[e];
      if (r / dy != e / dy && r % dy != e % dy) d++; else s++;
      e = r;
    }
    w.entry[c] = e; w.st[c] = s; w.dg[c] = d; w.hill[c] = in.wet[e] ? HILL_NONE : seg[e];
    if (e == c) continue;
    w.hand[c] = height(c) - height(e);
    if (w.hill[c] == HILL_NONE) continue;
    HillRec& r = w.recs[w.hill[c]];
    if (r.cells == 0u || s + d > r.steps_max) { r.steps_max = s + d; r.farthest_cell = c; }
    if (r.cells == 0u || w.hand[c] > r.hand_max) r.hand_max = w.hand[c];   // (finite and positive in these inputs)
    r.cells++; r.straight_sum += s; r.diagonal_sum += d;
    const uint64_t q = (uint64_t)floor(w.hand[c] * 1099511627776.0);   // (below 2^24 in these inputs; the cone's sums wrap)
    if (r.hand_sum_q40 + q < q) r.flags |= HILL_F_HAND;
    r.hand_sum_q40 += q;
    if (s + d == 1u) r.bank_cells++;
    if (e == r.first_cell) r.head_cells++;
  }
  return w;
}

static int check(const char* name, const std::vector<Input>& ins) {
  std::vector<dh_map*> maps;
  size_t words = 0;
  for (const Input& in : ins) { maps.push_back(host_map(in)); words += in.h.size(); }
  const uint32_t nm = (uint32_t)ins.size();
  int bad = 0;
  size_t shown = 0;
  for (uint32_t threshold : {1u, 3u, 40u}) {
    std::vector<Want> wants;
    uint32_t most = 0;
    for (uint32_t i = 0; i < nm; i++) { wants.push_back(plain(ins[i], maps[i], threshold)); most = std::max<uint32_t>(most, (uint32_t)wants.back().recs.size()); }
    if (threshold == 3u) shown = wants[0].recs.size();
    for (int v = 0; v < dh_variants(); v++)
      for (uint32_t lanes : {64u, 256u})
        for (int order = 0; order < 4; order++) {
          const uint32_t cap = order == 1 ? most / 2u : most + 2u;   // (one launch order with fewer records than segments)
          std::vector<uint32_t> ns(nm, 0), e(words), hl(words), st(words), dg(words);
          std::vector<double> hd(words);
          std::vector<HillRec> out((size_t)nm * cap + 1u);
          if (hh_hillslopes(maps.data(), nm, v, lanes, order, threshold, cap, out.data(), ns.data(), e.data(), hl.data(), st.data(), dg.data(), hd.data(), nullptr) != 0) { bad++; continue; }
          bool ok = true;
          size_t at = 0;
          for (uint32_t i = 0; i < nm && ok; i++) {
            const Want& w = wants[i];
            ok = ns[i] == w.recs.size() && std::equal(w.entry.begin(), w.entry.end(), e.begin() + at) && std::equal(w.hill.begin(), w.hill.end(), hl.begin() + at) &&
                 std::equal(w.st.begin(), w.st.end(), st.begin() + at) && std::equal(w.dg.begin(), w.dg.end(), dg.begin() + at) && same_bits(w.hand, hd.data() + at);
            const size_t k = std::min<size_t>(cap, w.recs.size());
            ok = ok && (k == 0 || memcmp(out.data() + (size_t)i * cap, w.recs.data(), k * sizeof(HillRec)) == 0);
            at += w.entry.size();
          }
          if (!ok) { printf("FAIL %s threshold %u variant %d lanes %u order %d\n", name, threshold, v, lanes, order); bad++; }
        }
  }
  for (dh_map* m : maps) dh_destroy(m);
  printf("%-10s %zu map(s), %5zu segments in the first at threshold 3  %s\n", name, ins.size(), shown, bad ? "FAILED" : "ok");
  return bad;
}

static int check_dump(const char* path) {
  Columns in;
  uint32_t tn[2] = {0, 0};
  std::vector<uint32_t> e, hl, st, dg;
  std::vector<double> hd;
  std::vector<HillRec> recs;
  if (!read_dump(path, 0x4C4C4948u, in, [&](FILE* f) {
        const size_t n = in.cells;
        return fread(tn, 4, 2, f) == 2 && tn[0] >= 1u && tn[1] <= n && take(f, e, n) && take(f, hl, n) && take(f, st, n) && take(f, dg, n) && take(f, hd, n) &&
               take(f, recs, tn[1]);
      })) return 1;
  const size_t n = in.cells;
  const uint32_t threshold = tn[0], ns = tn[1];
  dh_map* h = in.map();
  int bad = 0;
  for (int v = 0; v < dh_variants(); v++)
    for (uint32_t lanes : {64u, 256u})
      for (int order : {0, 3}) {
        uint32_t got = 0;
        std::vector<uint32_t> a(n), b(n), c(n), d(n);
        std::vector<double> g(n);
        std::vector<HillRec> out((size_t)ns + 2u);
        memset(out.data(), 0, out.size() * sizeof(HillRec));
        const bool same = hh_hillslopes(&h, 1, v, lanes, order, threshold, ns + 2u, out.data(), &got, a.data(), b.data(), c.data(), d.data(), g.data(), nullptr) == 0 &&
                          got == ns && a == e && b == hl && c == st && d == dg && same_bits(hd, g.data()) &&
                          (ns == 0 || memcmp(out.data(), recs.data(), (size_t)ns * sizeof(HillRec)) == 0);
        if (!same) { printf("FAIL %s variant %d lanes %u order %d: %u segments, expected %u\n", path, v, lanes, order, got, ns); bad++; }
      }
  dh_destroy(h);
  printf("%-36s %4ux%-4u threshold %4u %6u segments  %s\n", file_name(path), in.dimx, in.dimy, threshold, ns, bad ? "FAILED" : "ok");
  return bad;
}

int main(int argc, char** argv) {
  return check_main(argc, argv, check_dump, {"cone", "ramp", "plateau", "random", "lakes"}, {{"lakes", 33, 47}, {"cone", 70, 1}, {"random", 1, 70}},
                    [](const char* name, const std::vector<MapSpec>& specs) { return check(name, make_all(specs)); });
}
