// strata_check -- a stand-alone run of the strata readers' bodies for the sanitizers (tests/test_strata_host.py builds and runs it):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o strata_check strata_check.cpp && ./strata_check
// Drawn columns (empty ones, depths up to 40, a few of 300; types 0..9, 63, 64 and 70; sizes with NaN, -1 and 2^24 among them) at
// 1 x 1, 5 x 7, 33 x 47 and 96 x 80, workgroups of 64 and 256 lanes, one workgroup, a strided grid and more workgroups than cells:
// the totals, the thickness planes and the cores against plain loops over the columns; then a link out of the pool and a cycle,
// which must return -5 and write nothing. Exit status 0 = all equal.
#include <cstdio>
#include <cstdlib>

#include "strata_host.cpp"

struct Columns {
  int dx, dy;
  std::vector<uint32_t> count, type;
  std::vector<double> size, floor, sat;
};
static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t draw(uint32_t n) { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return (uint32_t)((g_seed >> 20) % n); }
static Columns columns(int dx, int dy) {
  Columns c;
  c.dx = dx; c.dy = dy;
  const uint32_t kinds[13] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 70};
  const double odd[4] = {NAN, -1.0, 16777216.0, -0.0};
  for (int i = 0; i < dx * dy; i++) {
    uint32_t k = draw(8) == 0 ? 0u : 1u + draw(40);
    if (draw(97) == 0) k = 300u;
    c.count.push_back(k);
    double base = 0.0;
    for (uint32_t j = 0; j < k; j++) {
      const double sz = draw(50) == 0 ? odd[draw(4)] : (double)(1u + draw(1u << 20)) * (1.0 / 1048576.0);
      c.type.push_back(kinds[draw(13)]); c.size.push_back(sz); c.floor.push_back(base); c.sat.push_back(draw(3) ? 0.0 : (double)draw(1000) * 0.001);
      if (sz == sz && sz > 0.0) base += sz;
    }
  }
  return c;
}
static bool same(const double* a, const double* b, size_t n) { return n == 0 || memcmp(a, b, n * 8) == 0; }

static int check(int dx, int dy) {
  const Columns c = columns(dx, dy);
  const size_t n = (size_t)dx * dy;
  std::vector<size_t> first(n + 1, 0);
  for (size_t i = 0; i < n; i++) first[i + 1] = first[i] + c.count[i];
  sh_map* h = sh_create(dx, dy, c.count.data(), c.type.data(), c.size.data(), c.floor.data(), c.sat.data(), 1, 3);
  int bad = 0;
  // plain loops
  const uint32_t NT = 64;
  std::vector<StrataRec> want(NT);
  memset(want.data(), 0, NT * sizeof(StrataRec));
  uint64_t wother = 0;
  const uint32_t list[4] = {1, 2, 0, 64};
  std::vector<double> wth(4 * n, 0.0), wcv(4 * n, -1.0);
  std::vector<uint32_t> wns(4 * n, 0u);
  for (size_t i = 0; i < n; i++) {
    uint64_t seen = 0;
    double run = 0.0;
    for (size_t k = first[i + 1]; k-- > first[i];) {
      const uint32_t t = c.type[k];
      for (int j = 0; j < 4; j++)
        if (t == list[j]) { if (!wns[j * n + i]) wcv[j * n + i] = run; wth[j * n + i] += c.size[k]; wns[j * n + i]++; }
      run += c.size[k];
      if (t >= NT) { wother++; continue; }
      StrataRec& r = want[t];
      if (k + 1 == first[i + 1]) r.top_cells++;
      r.sections++;
      if (!(seen >> t & 1)) { r.cells++; seen |= 1ull << t; }
      const double v = c.size[k], hd = c.size[k] * c.sat[k];
      if (!(v >= 0.0) || !(v < 16777216.0)) r.flags |= 1u; else r.volume_q40 += (uint64_t)floor(v * 1099511627776.0);
      if (!(hd >= 0.0) || !(hd < 16777216.0)) r.flags |= 2u; else r.held_q40 += (uint64_t)floor(hd * 1099511627776.0);
    }
  }
  std::vector<uint32_t> cells;
  for (size_t i = 0; i < n; i++) cells.push_back((uint32_t)i);
  for (size_t i = 0; i < n; i += 3) cells.push_back((uint32_t)(n - 1 - i));   // repeats, backwards
  uint64_t wtotal = 0;
  for (uint32_t cl : cells) wtotal += c.count[cl];
  const uint32_t shapes[5][2] = {{64, 1}, {64, 3}, {64, 500}, {256, 1}, {256, 4}};
  for (const auto& s : shapes) {
    std::vector<StrataRec> got(NT);
    uint64_t other = 7, info[2] = {0, 0};
    bool ok = sh_totals(&h, 1, s[0], s[1], NT, got.data(), &other, nullptr, info) == 0 && other == wother && memcmp(got.data(), want.data(), NT * sizeof(StrataRec)) == 0;
    std::vector<double> th(4 * n), cv(4 * n);
    std::vector<uint32_t> ns(4 * n);
    uint64_t cell = 0;
    ok = ok && sh_thickness(h, s[0], s[1], list, 4, th.data(), cv.data(), ns.data(), &cell) == 0 && same(th.data(), wth.data(), 4 * n) && same(cv.data(), wcv.data(), 4 * n) && ns == wns;
    std::vector<uint32_t> cnt(cells.size()), ty(wtotal);
    std::vector<double> sz(wtotal), fl(wtotal), st(wtotal);
    uint64_t total = 0;
    ok = ok && sh_cores(h, s[0], s[1], cells.data(), (uint32_t)cells.size(), cnt.data(), wtotal, &total, ty.data(), sz.data(), fl.data(), st.data(), &cell) == 0 && total == wtotal;
    size_t at = 0;
    for (size_t i = 0; ok && i < cells.size(); i++) {
      const size_t f = first[cells[i]], k = c.count[cells[i]];
      ok = cnt[i] == k && (k == 0 || memcmp(&ty[at], &c.type[f], k * 4) == 0) && same(&sz[at], &c.size[f], k) && same(&fl[at], &c.floor[f], k) && same(&st[at], &c.sat[f], k);
      at += k;
    }
    if (wtotal) ok = ok && sh_cores(h, s[0], s[1], cells.data(), (uint32_t)cells.size(), cnt.data(), wtotal - 1, &total, nullptr, nullptr, nullptr, nullptr, &cell) == 1 && total == wtotal;
    if (!ok) { printf("FAIL %dx%d lanes %u workgroups %u\n", dx, dy, s[0], s[1]); bad++; }
  }
  // corrupt chains: the deepest column gets a link out of the pool, then a cycle
  size_t deep = 0;
  for (size_t i = 0; i < n; i++) if (c.count[i] > c.count[deep]) deep = i;
  if (c.count[deep] >= 3) {
    for (int kind = 0; kind < 2; kind++) {
      const uint32_t top = sh_prev(h, 0, deep, 0, 0), second = sh_prev(h, 1, top, 0, 0);
      sh_prev(h, 1, top, 1, kind == 0 ? (uint32_t)sh_pool_size(h) : top);   // (kind 1: the section under the top points at itself)
      StrataRec one;
      memset(&one, 0x5A, sizeof(one));
      const StrataRec keep = one;
      uint64_t info[2] = {9, 9}, cell = 9, total = 9;
      double d = 5.0;
      uint32_t u = 5u, cl = (uint32_t)deep;
      bool ok = sh_totals(&h, 1, 64, 2, 1, &one, nullptr, nullptr, info) == -5 && info[1] == deep && memcmp(&one, &keep, sizeof(one)) == 0;
      ok = ok && sh_thickness(h, 256, 2, list, 1, &d, &d, &u, &cell) == -5 && cell == deep && d == 5.0 && u == 5u;
      cell = 9;
      ok = ok && sh_cores(h, 64, 2, &cl, 1, &u, 1000, &total, &u, &d, &d, &d, &cell) == -5 && cell == deep && total == 9 && u == 5u && d == 5.0;
      sh_prev(h, 1, top, 1, second);
      if (!ok) { printf("FAIL %dx%d corrupt chain kind %d\n", dx, dy, kind); bad++; }
    }
  }
  sh_destroy(h);
  printf("%3dx%-3d %7zu sections  %s\n", dx, dy, first[n], bad ? "FAILED" : "ok");
  return bad;
}

int main() {
  int bad = 0;
  const int dims[4][2] = {{1, 1}, {5, 7}, {33, 47}, {96, 80}};
  for (const auto& d : dims) bad += check(d[0], d[1]);
  return bad ? 1 : 0;
}
