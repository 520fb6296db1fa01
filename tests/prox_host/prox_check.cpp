// prox_check -- a stand-alone run of the proximity bodies for the sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o prox_check prox_check.cpp && ./prox_check
// Random heights under a Bernoulli(0.2) wet mask and an all-dry map at 33 x 47, 96 x 80, 1 x 70 and 70 x 1, and three maps in one
// call, every tile shape, 64 and 256 lanes, the four launch orders, the envelopes in 1, 3, 100 and the library's bands of columns. WATER mode (on the all-dry map: no site, no record, every plane
// 0xFFFFFFFF) and three lists -- one cell, every 7th cell in descending order, every cell -- with 0, 1 and 64 bins of width 1 and 3,
// against one plain loop per cell over ALL sites (the smallest d2 * 2^32 + site), the lakes found by a flood fill in cell order, the
// records and rows summed in cell order. Exit status 0 = all equal.
#include "prox_host.cpp"
#include "../analysis_host/analysis_check.h"

struct Want { std::vector<uint32_t> nearest, group, dist2, hist; std::vector<ProxRec> recs; };

// the rank of every wet cell's lake (eight neighbours, ranks in the order of the lakes' smallest cells), PROX_NONE for a dry cell
static std::vector<uint32_t> lake_ranks(const Input& in) {
  const size_t n = in.h.size();
  std::vector<uint32_t> rank(n, PROX_NONE), stack;
  uint32_t next = 0;
  for (size_t c0 = 0; c0 < n; c0++) {
    if (!in.wet[c0] || rank[c0] != PROX_NONE) continue;
    rank[c0] = next; stack.push_back((uint32_t)c0);
    while (!stack.empty()) {
      const uint32_t c = stack.back(); stack.pop_back();
      const int x = (int)(c / in.dy), y = (int)(c % in.dy);
      for (int dx = -1; dx <= 1; dx++)
        for (int dy = -1; dy <= 1; dy++) {
          const int u = x + dx, v = y + dy;
          if (u < 0 || v < 0 || u >= in.dx || v >= in.dy) continue;
          const size_t d = (size_t)u * in.dy + v;
          if (in.wet[d] && rank[d] == PROX_NONE) { rank[d] = next; stack.push_back((uint32_t)d); }
        }
    }
    next++;
  }
  return rank;
}

// mark: the group of every site, PROX_NONE elsewhere; ngroups: the records
static Want plain(const Input& in, const std::vector<uint32_t>& mark, uint32_t ngroups, uint32_t nbins, uint32_t bin_width) {
  const size_t n = in.h.size();
  const int64_t dy = in.dy;
  std::vector<uint32_t> sites;
  for (size_t c = 0; c < n; c++) if (mark[c] != PROX_NONE) sites.push_back((uint32_t)c);
  Want w;
  w.nearest.assign(n, PROX_NONE); w.group.assign(n, PROX_NONE); w.dist2.assign(n, PROX_NONE); w.hist.assign((size_t)ngroups * nbins, 0u);
  w.recs.resize(ngroups);
  if (ngroups) memset(w.recs.data(), 0, ngroups * sizeof(ProxRec));
  for (uint32_t g = 0; g < ngroups; g++) { w.recs[g].site = PROX_NONE; w.recs[g].x0 = w.recs[g].y0 = 0xFFFF; }
  for (size_t c = 0; c < n && !sites.empty(); c++) {
    const int64_t x = (int64_t)c / dy, y = (int64_t)c % dy;
    uint64_t best = ~0ull;
    for (uint32_t s : sites) {
      const int64_t ex = x - (int64_t)s / dy, ey = y - (int64_t)s % dy;
      best = std::min(best, ((uint64_t)(ex * ex + ey * ey) << 32) | s);
    }
    const uint32_t d2 = (uint32_t)(best >> 32), s = (uint32_t)best, g = mark[s];
    w.nearest[c] = s; w.dist2[c] = d2; w.group[c] = g;
    ProxRec& r = w.recs[g];
    if (d2 == 0) { r.sites++; r.site = std::min(r.site, (uint32_t)c); }
    if (r.cells == 0 || d2 > r.dist2_max) { r.dist2_max = d2; r.farthest_cell = (uint32_t)c; }   // (ascending c: of equals the first stays)
    r.cells++; r.dist2_sum += d2;
    if (x == 0 || y == 0 || x == in.dx - 1 || y == in.dy - 1) r.flags |= PROX_F_BORDER;
    r.x0 = std::min<uint16_t>(r.x0, (uint16_t)x); r.x1 = std::max<uint16_t>(r.x1, (uint16_t)x);
    r.y0 = std::min<uint16_t>(r.y0, (uint16_t)y); r.y1 = std::max<uint16_t>(r.y1, (uint16_t)y);
    if (nbins) {
      uint32_t root = 0;
      while ((uint64_t)(root + 1u) * (root + 1u) <= d2) root++;
      w.hist[(size_t)g * nbins + std::min(root / bin_width, nbins - 1u)]++;
    }
  }
  return w;
}

static int check(const char* name, const std::vector<Input>& ins) {
  std::vector<dh_map*> maps;
  size_t words = 0, least = ~(size_t)0;
  for (const Input& in : ins) { maps.push_back(host_map(in)); words += in.h.size(); least = std::min(least, in.h.size()); }
  const uint32_t nm = (uint32_t)ins.size();
  int bad = 0;
  std::vector<std::vector<uint32_t>> lists(4);   // (lists[0]: WATER mode)
  lists[1] = {(uint32_t)(least / 2)};
  for (uint32_t c = 0; c < least; c += 7) lists[2].push_back((uint32_t)(least - 1 - c));   // (descending: positions are not cell order)
  for (uint32_t c = 0; c < least; c++) lists[3].push_back(c);
  for (size_t li = 0; li < lists.size(); li++) {
    const std::vector<uint32_t>& list = lists[li];
    const uint32_t n = (uint32_t)list.size(), nbins = li == 1 ? 1u : li == 2 ? 64u : li == 0 ? 5u : 0u, bw = li == 0 ? 3u : 1u;
    std::vector<Want> wants;
    uint32_t cap = n;
    for (uint32_t i = 0; i < nm; i++) {
      std::vector<uint32_t> mark(ins[i].h.size(), PROX_NONE);
      uint32_t groups = n;
      if (li == 0) {
        mark = lake_ranks(ins[i]);
        groups = 0;
        for (uint32_t r : mark) if (r != PROX_NONE) groups = std::max(groups, r + 1u);
      } else {
        for (uint32_t k = 0; k < n; k++) mark[list[k]] = k;
      }
      wants.push_back(plain(ins[i], mark, groups, nbins, bw));
      if (li == 0) cap = std::max(cap, groups);
    }
    for (int v = 0; v < dh_variants(); v++)
      for (uint32_t lanes : {64u, 256u})
        for (int order : {0, 1, 2, 3}) {
          const uint32_t bands = order == 0 ? 1u : order == 1 ? ph_bands() : order == 2 ? 3u : 100u;   // (100: a band per column on the narrow maps)
          std::vector<uint32_t> nr(words), gr(words), d2(words), hist((size_t)nm * cap * nbins + 1u, 0xDEADBEEFu), counts(nm + 1u, 0xDEADBEEFu);
          std::vector<ProxRec> out((size_t)nm * cap + 1u);
          memset(out.data(), 0xEE, out.size() * sizeof(ProxRec));
          if (ph_proximity(maps.data(), nm, v, lanes, order, n ? list.data() : nullptr, n, cap ? out.data() : nullptr, sizeof(ProxRec), cap, counts.data(),
                           nbins ? hist.data() : nullptr, nbins, bw, nr.data(), gr.data(), d2.data(), bands) != 0) { bad++; continue; }
          bool ok = hist.back() == 0xDEADBEEFu && out.back().site == 0xEEEEEEEEu && counts.back() == 0xDEADBEEFu;   // (nothing behind what was asked for)
          size_t at = 0;
          for (uint32_t i = 0; i < nm && ok; i++) {
            const Want& w = wants[i];
            const size_t cells = ins[i].h.size(), nrec = w.recs.size();
            ok = counts[i] == nrec && std::equal(w.nearest.begin(), w.nearest.end(), nr.begin() + at) && std::equal(w.group.begin(), w.group.end(), gr.begin() + at) &&
                 std::equal(w.dist2.begin(), w.dist2.end(), d2.begin() + at) && w.nearest.size() == cells &&
                 std::equal(w.hist.begin(), w.hist.end(), hist.begin() + (size_t)i * cap * nbins) &&
                 (nrec == 0 || memcmp(out.data() + (size_t)i * cap, w.recs.data(), nrec * sizeof(ProxRec)) == 0);
            for (size_t r = nrec; r < cap && ok; r++) ok = out[(size_t)i * cap + r].site == 0xEEEEEEEEu;   // (the records a map does not have stay untouched)
            at += cells;
          }
          if (!ok) { printf("FAIL %s list %zu variant %d lanes %u order %d\n", name, li, v, lanes, order); bad++; }
        }
  }
  for (dh_map* m : maps) dh_destroy(m);
  printf("%-10s %zu map(s)  %s\n", name, ins.size(), bad ? "FAILED" : "ok");
  return bad;
}

int main() {
  int bad = 0;
  const int dims[4][2] = {{33, 47}, {96, 80}, {1, 70}, {70, 1}};
  for (const auto& d : dims)
    for (const char* kind : {"lakes", "random"}) bad += check(kind, make_all({{kind, d[0], d[1]}}));   // ("random": no wet cell, WATER mode has no site)
  bad += check("three maps", make_all({{"lakes", 33, 47}, {"random", 70, 1}, {"lakes", 1, 70}}));
  return bad ? 1 : 0;
}
