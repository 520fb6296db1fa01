// flowpaths_check -- a stand-alone run of the flow path bodies for the sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o flowpaths_check flowpaths_check.cpp && ./flowpaths_check
// Without arguments: a ramp, a plateau, random heights and random heights under a Bernoulli(0.2) wet mask at 33 x 47 and 96 x 80, and
// three maps in one call, every tile shape, 64 and 256 lanes, the four launch orders and the up-walk against them, against two plain
// walks per cell down the receivers of the drainage host build (the seven planes per cell, the profile, the records field by field),
// with caps above and below the counts.
// With arguments: each names a dump written by tests/test_flowpaths_host.py -- the hand-built map, the spiral or another input of
// tests/drainage_ref.py with the restatement's result: the columns' top records exactly as the snapshot holds them, then the counts,
// the seven planes, the profile and the records, all compared bit by bit. Every tile shape, 64 and 256 lanes, workgroups and lanes
// first to last and last to first. Little-endian words:
//   u32 magic 0x48544150, i32 dimx, i32 dimy, u32 nsec, u32 count[cells], u32 type[nsec], f64 size[nsec], f64 floor[nsec],
//   u32 nbasins, u32 nprofile, u32 terminal[cells], u32 straight[cells], u32 diagonal[cells], f64 drop[cells], u32 upstream[cells],
//   u32 source[cells], u32 stem[cells], u32 profile[nprofile], 64-byte records[nbasins]
// Exit status 0 = all equal.
#include "flowpaths_host.cpp"
#include "../analysis_host/analysis_check.h"

struct Want { std::vector<uint32_t> term, st, dg, ups, src, stem, prof; std::vector<double> drop; std::vector<PathRec> recs; };

// two walks per cell down the receivers: the steps, then the key left at every cell passed; the records summed in cell order
static Want plain(const Input& in, dh_map* h) {
  const size_t n = in.h.size();
  const uint32_t dy = (uint32_t)in.dy;
  uint32_t nb = 0;
  std::vector<uint32_t> recv(n), lab(n);
  std::vector<BasinRec> brec(n + 1);
  if (dh_drainage(&h, 1, 0, 256, 0, (uint32_t)n, brec.data(), &nb, recv.data(), lab.data(), nullptr) != 0) exit(2);
  auto height = [&](size_t c) { return in.wet[c] ? in.h[c] + 0.5 : in.h[c]; };
  Want w;
  w.term.assign(n, 0u); w.st.assign(n, 0u); w.dg.assign(n, 0u); w.ups.assign(n, 0u); w.src.assign(n, 0u); w.stem.assign(n, PATH_NONE); w.drop.assign(n, 0.0);
  std::vector<uint64_t> up(n, 0ull), far(nb, 0ull);
  for (uint32_t c = 0; c < n; c++) {
    uint32_t e = c, s = 0, d = 0;
    while (recv[e] != DRAIN_NONE) {
      const uint32_t r = recv[e];
      if (r / dy != e / dy && r % dy != e % dy) d++; else s++;
      e = r;
    }
    w.term[c] = e; w.st[c] = s; w.dg[c] = d;
    if (e != c) w.drop[c] = height(c) - height(e);
  }
  for (uint32_t c = 0; c < n; c++) {
    const uint64_t k = ((uint64_t)(w.st[c] + w.dg[c]) << 32) | (uint64_t)(0xFFFFFFFFu - c);
    far[lab[c]] = std::max(far[lab[c]], k);
    for (uint32_t e = c;; e = recv[e]) {
      up[e] = std::max(up[e], k);
      if (recv[e] == DRAIN_NONE) break;
    }
  }
  w.recs.resize(nb);
  uint32_t at = 0;
  for (uint32_t b = 0; b < nb; b++) {
    PathRec& r = w.recs[b];
    memset(&r, 0, sizeof(r));
    r.first_cell = brec[b].first_cell; r.steps_max = (uint32_t)(far[b] >> 32); r.source_cell = 0xFFFFFFFFu - (uint32_t)far[b];
    r.terminal_cell = w.term[r.source_cell]; r.diagonal = w.dg[r.source_cell]; r.profile_at = at; r.flags = in.wet[r.terminal_cell] ? PATH_F_WET : 0u;
    r.drop_source = w.drop[r.source_cell];
    at += r.steps_max + 1u;
  }
  w.prof.assign(at, PATH_NONE);
  for (uint32_t c = 0; c < n; c++) {
    PathRec& r = w.recs[lab[c]];
    const uint32_t steps = w.st[c] + w.dg[c];
    w.ups[c] = (uint32_t)(up[c] >> 32) - steps; w.src[c] = 0xFFFFFFFFu - (uint32_t)up[c];
    if (up[c] == far[lab[c]]) { w.stem[c] = r.steps_max - steps; w.prof[r.profile_at + w.stem[c]] = c; }
    r.cells++; r.straight_sum += w.st[c]; r.diagonal_sum += w.dg[c];
    if (w.drop[c] > r.drop_max) r.drop_max = w.drop[c];   // (finite and not negative in these inputs)
  }
  return w;
}

static int check(const char* name, const std::vector<Input>& ins) {
  std::vector<dh_map*> maps;
  size_t words = 0;
  for (const Input& in : ins) { maps.push_back(host_map(in)); words += in.h.size(); }
  const uint32_t nm = (uint32_t)ins.size();
  int bad = 0;
  std::vector<Want> wants;
  uint32_t most = 0;
  for (uint32_t i = 0; i < nm; i++) { wants.push_back(plain(ins[i], maps[i])); most = std::max<uint32_t>(most, (uint32_t)wants.back().recs.size()); }
  for (int v = 0; v < dh_variants(); v++)
    for (uint32_t lanes : {64u, 256u})
      for (int order : {0, 1, 2, 3, 4, 8, 13}) {
        const uint32_t cap = order == 1 ? most / 2u : most + 2u;   // (one launch order with fewer records than basins)
        const uint32_t npw = (uint32_t)wants[0].prof.size();
        const uint32_t pcap = nm != 1 ? 0u : order == 2 ? npw / 2u : npw + 3u;   // (... and one with a shorter profile)
        std::vector<uint32_t> ns(nm, 0), np(nm, 0), t(words), st(words), dg(words), us(words), sr(words), sm(words), pr((size_t)pcap + 1u, 0xDEADBEEFu);
        std::vector<double> dr(words);
        std::vector<PathRec> out((size_t)nm * cap + 1u);
        if (fh_flowpaths(maps.data(), nm, v, lanes, order, cap, out.data(), ns.data(), t.data(), st.data(), dg.data(), dr.data(), us.data(), sr.data(), sm.data(),
                         pcap ? pr.data() : nullptr, pcap, np.data(), nullptr) != 0) { bad++; continue; }
        bool ok = true;
        size_t at = 0;
        for (uint32_t i = 0; i < nm && ok; i++) {
          const Want& w = wants[i];
          ok = ns[i] == w.recs.size() && np[i] == w.prof.size() && std::equal(w.term.begin(), w.term.end(), t.begin() + at) &&
               std::equal(w.st.begin(), w.st.end(), st.begin() + at) && std::equal(w.dg.begin(), w.dg.end(), dg.begin() + at) && same_bits(w.drop, dr.data() + at) &&
               std::equal(w.ups.begin(), w.ups.end(), us.begin() + at) && std::equal(w.src.begin(), w.src.end(), sr.begin() + at) &&
               std::equal(w.stem.begin(), w.stem.end(), sm.begin() + at);
          const size_t k = std::min<size_t>(cap, w.recs.size());
          ok = ok && (k == 0 || memcmp(out.data() + (size_t)i * cap, w.recs.data(), k * sizeof(PathRec)) == 0);
          at += w.term.size();
        }
        const size_t pk = std::min<size_t>(pcap, npw);
        ok = ok && std::equal(pr.begin(), pr.begin() + pk, wants[0].prof.begin()) && pr[pk] == 0xDEADBEEFu;   // (nothing behind what was asked for)
        if (!ok) { printf("FAIL %s variant %d lanes %u order %d\n", name, v, lanes, order); bad++; }
      }
  for (dh_map* m : maps) dh_destroy(m);
  printf("%-10s %zu map(s), %5zu basins and a profile of %5zu cells in the first  %s\n", name, ins.size(), wants[0].recs.size(), wants[0].prof.size(), bad ? "FAILED" : "ok");
  return bad;
}

static int check_dump(const char* path) {
  Columns in;
  uint32_t tn[2] = {0, 0};
  std::vector<uint32_t> t, st, dg, us, sr, sm, pr;
  std::vector<double> dr;
  std::vector<PathRec> recs;
  if (!read_dump(path, 0x48544150u, in, [&](FILE* f) {
        const size_t n = in.cells;
        return fread(tn, 4, 2, f) == 2 && tn[0] <= n && tn[1] <= n && take(f, t, n) && take(f, st, n) && take(f, dg, n) && take(f, dr, n) && take(f, us, n) &&
               take(f, sr, n) && take(f, sm, n) && take(f, pr, tn[1]) && take(f, recs, tn[0]);
      })) return 1;
  const size_t n = in.cells;
  const uint32_t nb = tn[0], npw = tn[1];
  dh_map* h = in.map();
  int bad = 0;
  for (int v = 0; v < dh_variants(); v++)
    for (uint32_t lanes : {64u, 256u})
      for (int order : {0, 3, 6}) {
        uint32_t got = 0, gp = 0;
        std::vector<uint32_t> a(n), b(n), c(n), d(n), e(n), g(n), p((size_t)npw + 1u);
        std::vector<double> q(n);
        std::vector<PathRec> out((size_t)nb + 2u);
        memset(out.data(), 0, out.size() * sizeof(PathRec));
        const bool same = fh_flowpaths(&h, 1, v, lanes, order, nb + 2u, out.data(), &got, a.data(), b.data(), c.data(), q.data(), d.data(), e.data(), g.data(), p.data(),
                                       npw + 1u, &gp, nullptr) == 0 &&
                          got == nb && gp == npw && a == t && b == st && c == dg && same_bits(dr, q.data()) && d == us && e == sr && g == sm &&
                          std::equal(pr.begin(), pr.end(), p.begin()) && (nb == 0 || memcmp(out.data(), recs.data(), (size_t)nb * sizeof(PathRec)) == 0);
        if (!same) { printf("FAIL %s variant %d lanes %u order %d: %u basins, expected %u\n", path, v, lanes, order, got, nb); bad++; }
      }
  dh_destroy(h);
  printf("%-36s %4ux%-4u %6u basins, a profile of %6u cells  %s\n", file_name(path), in.dimx, in.dimy, nb, npw, bad ? "FAILED" : "ok");
  return bad;
}

int main(int argc, char** argv) {
  return check_main(argc, argv, check_dump, {"ramp", "plateau", "random", "lakes"}, {{"lakes", 33, 47}, {"random", 70, 1}, {"random", 1, 70}},
                    [](const char* name, const std::vector<MapSpec>& specs) { return check(name, make_all(specs)); });
}
