// dispersal_check -- a stand-alone run of the dispersed-flow bodies for the sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o dispersal_check dispersal_check.cpp && ./dispersal_check
// Without arguments: a ramp, a plateau, random heights and random heights under a Bernoulli(0.2) wet mask at 1 x 1, 2 x 3, 9 x 7 and
// 33 x 47, and three maps in one call, with exponents 0, 1 and 4, every tile shape, 64 and 256 lanes, the four launch orders, the flow
// launches against them and with one workgroup, against a plain accumulation in descending height over the receivers and labels of
// the drainage host build (the three planes per cell, the records field by field), with caps above and below the counts; a call
// without a map and an exponent of 17 are refused BY THIS HARNESS and write nothing. (That is not the library's empty ensemble: there
// analysis_begin returns 0 before any body runs, which only tests/test_gpu_dispersal.py sees; no body runs on an empty table here
// either.)
// With arguments: each names a dump written by tests/test_dispersal_host.py -- the hand-built map or another input of
// tests/drainage_ref.py with the restatement's result: the columns' top records exactly as the snapshot holds them, then the planes
// and the records, all compared bit by bit. Every tile shape, 64 and 256 lanes, workgroups and lanes first to last and last to first.
// Little-endian words:
//   u32 dimx, u32 dimy, u32 exponent, u32 nbasins, u32 count[cells], u32 nsec, u32 type[nsec], f64 size[nsec], f64 floor[nsec],
//   u64 area[cells], u32 donors[cells], u32 receivers[cells], 64-byte records[nbasins]
// Exit status 0 = all equal.
#include "dispersal_host.cpp"
#include "../analysis_host/analysis_check.h"

struct Want { std::vector<uint64_t> area; std::vector<uint32_t> donors, receivers; std::vector<DispRec> recs; };

// the definition in plain loops: the givers in descending height, every one complete when its turn comes
static Want plain(const Input& in, dh_map* h, uint32_t exponent) {
  const size_t n = in.h.size();
  const int dx = in.dx, dy = in.dy;
  uint32_t nb = 0;
  std::vector<uint32_t> recv(n), lab(n);
  std::vector<BasinRec> brec(n + 1);
  if (dh_drainage(&h, 1, 0, 256, 0, (uint32_t)n, brec.data(), &nb, recv.data(), lab.data(), nullptr) != 0) exit(2);
  auto height = [&](size_t c) { return in.wet[c] ? in.h[c] + 0.5 : in.h[c]; };
  Want w;
  w.area.assign(n, DISP_ONE); w.donors.assign(n, 0u); w.receivers.assign(n, 0u);
  std::vector<std::vector<uint32_t>> lower(n);
  for (uint32_t c = 0; c < n; c++) {
    if (in.wet[c]) continue;
    const int x = (int)c / dy, y = (int)c % dy;
    for (int u = x - 1; u <= x + 1; u++)
      for (int v = y - 1; v <= y + 1; v++) {
        if ((u == x && v == y) || u < 0 || v < 0 || u >= dx || v >= dy) continue;
        const uint32_t m = (uint32_t)(u * dy + v);
        if (height(m) < height(c)) { lower[c].push_back(m); w.donors[m]++; }
      }
    w.receivers[c] = (uint32_t)lower[c].size();
  }
  std::vector<uint32_t> order;
  for (uint32_t c = 0; c < n; c++) if (!lower[c].empty()) order.push_back(c);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return height(a) > height(b); });
  std::vector<uint64_t> lin(nb, 0ull), lout(nb, 0ull);
  for (uint32_t c : order) {
    std::vector<double> ws;
    double W = 0.0;
    for (uint32_t m : lower[c]) {
      const bool diag = m / (uint32_t)dy != c / (uint32_t)dy && m % (uint32_t)dy != c % (uint32_t)dy;
      const double s = (height(c) - height(m)) * (diag ? 0.7071067811865476 : 1.0);
      double p = 1.0;
      for (uint32_t e = 0; e < exponent; e++) p = p * s;
      ws.push_back(p);
      W = W + p;
    }
    const bool ok = W > 0.0 && std::isfinite(W);
    uint64_t sum = 0;
    std::vector<uint64_t> share;
    for (double p : ws) {
      const uint32_t f = ok ? (uint32_t)((p / W) * 16777216.0) : 0u;
      share.push_back((uint64_t)(((unsigned __int128)w.area[c] * f) >> 24));
      sum += share.back();
    }
    for (size_t i = 0; i < lower[c].size(); i++) {
      const uint32_t m = lower[c][i];
      const uint64_t amount = share[i] + (m == recv[c] ? w.area[c] - sum : 0ull);
      w.area[m] += amount;
      if (lab[m] != lab[c]) { lout[lab[c]] += amount; lin[lab[m]] += amount; }
    }
  }
  w.recs.resize(nb);
  for (uint32_t b = 0; b < nb; b++) {
    DispRec& r = w.recs[b];
    memset(&r, 0, sizeof(r));
    r.first_cell = brec[b].first_cell; r.cells = brec[b].cells; r.flags = brec[b].flags; r.peak_cell = DISP_NONE;
    r.leak_in_q24 = lin[b]; r.leak_out_q24 = lout[b];
  }
  for (uint32_t c = 0; c < n; c++) {
    DispRec& r = w.recs[lab[c]];
    if (recv[c] == DRAIN_NONE) r.inflow_q24 += w.area[c];
    if (!in.wet[c] && w.area[c] > r.peak_q24) { r.peak_q24 = w.area[c]; r.peak_cell = c; }   // (ascending c: the smallest cell stays)
    if (w.receivers[c]) r.givers++;
    if (w.receivers[c] >= 2) r.split_cells++;
  }
  return w;
}

// every shape, width and order of one call over `maps` against `wants`
static int compare(const char* name, std::vector<dh_map*>& maps, const std::vector<size_t>& cells, const std::vector<Want>& wants, uint32_t exponent, bool all_orders) {
  const uint32_t nm = (uint32_t)maps.size();
  size_t words = 0;
  uint32_t most = 0;
  for (uint32_t i = 0; i < nm; i++) { words += cells[i]; most = std::max<uint32_t>(most, (uint32_t)wants[i].recs.size()); }
  int bad = 0;
  for (int v = 0; v < dh_variants(); v++)
    for (uint32_t lanes : {64u, 256u})
      for (int order : {0, 1, 2, 3, 4, 8, 12, 7}) {
        if (!all_orders && order != 0 && order != 3) continue;
        for (uint32_t blocks : {1024u, 1u, 3u}) {
          if (blocks != 1024u && order != 0 && order != 12) continue;
          for (uint32_t cap : {most + 2u, most > 1u ? most - 1u : 0u, 0u}) {
            if (cap != most + 2u && (v != 0 || order != 0)) continue;
            std::vector<DispRec> out((size_t)nm * cap + 1);
            std::vector<uint32_t> nb(nm), donors(words), receivers(words);
            std::vector<uint64_t> area(words);
            uint32_t rounds = 0;
            const int rc = dph_dispersal(maps.data(), nm, v, lanes, order, blocks, exponent, cap, cap ? out.data() : nullptr, nb.data(), area.data(), donors.data(),
                                         receivers.data(), &rounds);
            bool ok = rc == 0;
            size_t at = 0;
            for (uint32_t i = 0; ok && i < nm; i++) {
              const Want& w = wants[i];
              ok = nb[i] == w.recs.size() && !memcmp(area.data() + at, w.area.data(), cells[i] * 8) && !memcmp(donors.data() + at, w.donors.data(), cells[i] * 4) &&
                   !memcmp(receivers.data() + at, w.receivers.data(), cells[i] * 4);
              const uint32_t k = std::min<uint32_t>(cap, nb[i]);
              for (uint32_t r = 0; ok && r < k; r++) ok = !memcmp(&out[(size_t)i * cap + r], &w.recs[r], sizeof(DispRec));
              at += cells[i];
            }
            if (!ok) {
              printf("%s exponent %u: variant %d lanes %u order %d flow workgroups %u cap %u: rc %d, differs\n", name, exponent, v, lanes, order, blocks, cap, rc);
              bad++;
            }
          }
        }
      }
  return bad;
}

static int check(const char* name, const std::vector<Input>& ins) {
  int bad = 0;
  std::vector<dh_map*> maps;
  std::vector<size_t> cells;
  for (const Input& in : ins) { maps.push_back(host_map(in)); cells.push_back(in.h.size()); }
  for (uint32_t exponent : {0u, 1u, 4u}) {
    std::vector<Want> wants;
    for (size_t i = 0; i < ins.size(); i++) wants.push_back(plain(ins[i], maps[i], exponent));
    bad += compare(name, maps, cells, wants, exponent, true);
  }
  for (dh_map* m : maps) dh_destroy(m);
  return bad;
}

// (this dump has a head of its own, not the common one of analysis_check.h: no magic word, the exponent and the count in front)
static int check_dump(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { printf("%s: cannot open\n", path); return 1; }
  std::vector<uint32_t> head, count, nsec, type;
  std::vector<double> size, floor;
  Want w;
  bool ok = take(f, head, 4);
  const size_t n = ok ? (size_t)head[0] * head[1] : 0;
  ok = ok && take(f, count, n) && take(f, nsec, 1) && take(f, type, nsec[0]) && take(f, size, nsec[0]) && take(f, floor, nsec[0]);
  ok = ok && take(f, w.area, n) && take(f, w.donors, n) && take(f, w.receivers, n) && take(f, w.recs, head[3]);
  fclose(f);
  if (!ok) { printf("%s: short file\n", path); return 1; }
  std::vector<dh_map*> maps{dh_create((int)head[0], (int)head[1], count.data(), type.data(), size.data(), floor.data())};
  const int bad = compare(path, maps, {n}, {w}, head[2], false);
  dh_destroy(maps[0]);
  return bad;
}

int main(int argc, char** argv) {
  int bad = 0;
  if (argc > 1) {
    for (int i = 1; i < argc; i++) bad += check_dump(argv[i]);
    if (bad) { printf("dispersal_check: %d differences\n", bad); return 1; }
    printf("dispersal_check: OK (%d files)\n", argc - 1);
    return 0;
  }
  for (const char* kind : {"ramp", "plateau", "random", "lakes"}) {
    for (auto d : {std::pair<int, int>{1, 1}, {2, 3}, {9, 7}, {33, 47}}) bad += check(kind, {make(kind, d.first, d.second)});
  }
  bad += check("three maps", {make("lakes", 33, 47), make("random", 1, 1), make("ramp", 9, 7)});
  {   // many tiny members: together they have more working member-launches than a batch has launches
    std::vector<Input> tiny;
    for (int i = 0; i < 8; i++) tiny.push_back(make("ramp", 1, 20));
    tiny.push_back(make("ramp", 5, 5));
    bad += check("nine tiny ramps", tiny);
  }
  {   // calls the harness refuses write nothing: no map at all, an exponent above 16
    Input in = make("random", 9, 7);
    dh_map* m = host_map(in);
    uint32_t nb = 7;
    if (dph_dispersal(nullptr, 0, 0, 256, 0, 1024, 1, 0, nullptr, &nb, nullptr, nullptr, nullptr, nullptr) != -2 || nb != 7) { printf("no map: not refused\n"); bad++; }
    if (dph_dispersal(&m, 1, 0, 256, 0, 1024, 17, 0, nullptr, &nb, nullptr, nullptr, nullptr, nullptr) != -2 || nb != 7) { printf("exponent 17: not refused\n"); bad++; }
    if (dph_dispersal(&m, 1, 0, 256, 0, 1024, 16, 0, nullptr, &nb, nullptr, nullptr, nullptr, nullptr) != 0 || nb == 7) { printf("exponent 16: refused\n"); bad++; }
    dh_destroy(m);
  }
  if (bad) { printf("dispersal_check: %d differences\n", bad); return 1; }
  printf("dispersal_check: OK\n");
  return 0;
}
