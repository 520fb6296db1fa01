// budget_check -- a stand-alone run of the sediment budget's bodies for the sanitizers (tests/test_budget_host.py builds and runs it):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o budget_check budget_check.cpp && ./budget_check
// Drawn pairs of maps (empty columns, depths up to 30, a few of 300; types 0..6, 31, 63, 64 and 70; sizes with NaN, -1 and 2^24 among
// them; a NaN floor here and there; "now" made of the base by redrawing, trimming, topping and emptying columns) at 1 x 1, 5 x 7,
// 33 x 47 and 96 x 80, every tile variant, workgroups of 64 and 256 lanes, workgroups and lanes first to last and last to first: the
// records, the soil table and the planes against plain loops over the columns (the basins' labels are the drainage host chain's own);
// three members against one base in one call; then a link out of the pool and a cycle, in the base and in a member, which must
// return -5, name the map and the cell and write nothing. Exit status 0 = all equal.
#include <cstdio>
#include <cstdlib>

#include "budget_host.cpp"

struct Columns {
  int dx, dy;
  std::vector<uint32_t> count, type;
  std::vector<double> size, floor, sat;
  std::vector<size_t> first;   // first section of each cell, and one past the last
};
static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t draw(uint32_t n) { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return (uint32_t)((g_seed >> 20) % n); }
static const uint32_t KINDS[11] = {0, 1, 2, 3, 4, 5, 6, 31, 63, 64, 70};
static void push_section(Columns& c, double& base) {
  const double odd[4] = {NAN, -1.0, 16777216.0, -0.0};
  const double sz = draw(60) == 0 ? odd[draw(4)] : (double)(1u + draw(1u << 20)) * (1.0 / 1048576.0);
  c.type.push_back(KINDS[draw(11)]); c.size.push_back(sz); c.floor.push_back(draw(200) == 0 ? NAN : base); c.sat.push_back(draw(3) ? 0.0 : (double)draw(1000) * 0.001);
  if (sz == sz && sz > 0.0 && sz < 1e6) base += sz;
}
static void index_columns(Columns& c) {
  c.first.assign(c.count.size() + 1, 0);
  for (size_t i = 0; i < c.count.size(); i++) c.first[i + 1] = c.first[i] + c.count[i];
}
static Columns columns(int dx, int dy) {
  Columns c;
  c.dx = dx; c.dy = dy;
  for (int i = 0; i < dx * dy; i++) {
    uint32_t k = draw(8) == 0 ? 0u : 1u + draw(30);
    if (draw(97) == 0) k = 300u;
    c.count.push_back(k);
    double base = (double)draw(64) * 0.125;
    for (uint32_t j = 0; j < k; j++) push_section(c, base);
  }
  index_columns(c);
  return c;
}
// "now": every column of `b` kept, redrawn, trimmed from the top, topped up or emptied
static Columns changed(const Columns& b) {
  Columns c;
  c.dx = b.dx; c.dy = b.dy;
  for (size_t i = 0; i < b.count.size(); i++) {
    const uint32_t how = draw(6);
    uint32_t keep = b.count[i];
    if (how == 1) keep = 0;
    if (how == 2 && keep) keep -= 1u + draw(keep);
    double base = 0.0;
    for (uint32_t j = 0; j < keep; j++) {
      const size_t k = b.first[i] + j;
      c.type.push_back(b.type[k]); c.size.push_back(b.size[k]); c.floor.push_back(b.floor[k]); c.sat.push_back(b.sat[k]);
      base = b.floor[k] + b.size[k];
    }
    if (!(base == base) || base > 1e6) base = 1.0;
    uint32_t more = how == 3 ? 1u + draw(4) : how == 1 ? draw(3) : 0u;
    if (how == 4 && keep) { c.size.back() *= 0.5; c.sat.back() = 0.25; }
    for (uint32_t j = 0; j < more; j++) push_section(c, base);
    c.count.push_back(keep + more);
  }
  index_columns(c);
  return c;
}
static bh_map* host_map(const Columns& c, int scramble) {
  return bh_create(c.dx, c.dy, c.count.data(), c.type.data(), c.size.data(), c.floor.data(), c.sat.data(), scramble, 3);
}

// ---- the plain restatement: per cell the sums of a column, then the records
struct Cell { uint32_t top; double ground, h; uint64_t v[71], x[71], solid; uint32_t f[71], fb; };
static uint64_t q40(double v, bool& ok) { ok = v >= 0.0 && v < 16777216.0; return ok ? (uint64_t)floor(v * 1099511627776.0) : 0ull; }
static void cell_of(const Columns& c, size_t i, Cell& o) {
  memset(&o, 0, sizeof(o));
  o.top = EMPTY;
  if (!c.count[i]) return;
  const size_t t = c.first[i + 1] - 1;
  o.top = c.type[t];
  o.ground = c.type[t] == 0 ? c.floor[t] : c.floor[t] + c.size[t];
  o.h = c.floor[t] + c.size[t];
  for (size_t k = c.first[i]; k <= t; k++) {
    const uint32_t ty = c.type[k];
    bool ok;
    const uint64_t qv = q40(c.size[k], ok);
    if (!ok) { o.f[ty] |= 1u; o.fb |= 1u; }
    if (o.v[ty] + qv < qv) { o.f[ty] |= 2u; if (ty == 0) o.fb |= 2u; }
    o.v[ty] += qv;
    if (ty != 0) { if (o.solid + qv < qv) o.fb |= 2u; o.solid += qv; }
    const uint64_t qh = q40(c.size[k] * c.sat[k], ok);
    if (!ok) o.f[ty] |= 1u;
    if (o.x[ty] + qh < qh) o.f[ty] |= 2u;
    o.x[ty] += qh;
  }
}
static void add(uint64_t& sum, uint64_t v, uint32_t& flags) { if (sum + v < v) flags |= 2u; sum += v; }

struct Want {
  std::vector<BudgetBasinRec> basins;
  std::vector<BudgetSoilRec> soils;
  std::vector<double> dg, dh;
  std::vector<int64_t> ds, dw;
};
static Want restate(const Columns& b, const Columns& n, const std::vector<BasinRec>& drain, const std::vector<uint32_t>& label, uint32_t ntypes) {
  Want w;
  const size_t cells = b.count.size();
  w.basins.resize(drain.size()); w.soils.resize(ntypes);
  memset(w.basins.data(), 0, w.basins.size() * sizeof(BudgetBasinRec)); memset(w.soils.data(), 0, w.soils.size() * sizeof(BudgetSoilRec));
  for (size_t k = 0; k < drain.size(); k++) {
    w.basins[k].first_cell = drain[k].first_cell; w.basins[k].cells = drain[k].cells; w.basins[k].cut_cell = w.basins[k].fill_cell = BUDGET_NONE;
  }
  w.dg.resize(cells); w.dh.resize(cells); w.ds.resize(cells); w.dw.resize(cells);
  static Cell cb, cn;
  for (size_t i = 0; i < cells; i++) {
    cell_of(b, i, cb); cell_of(n, i, cn);
    const double d = cn.ground - cb.ground;
    w.dg[i] = d; w.dh[i] = cn.h - cb.h;
    w.ds[i] = (int64_t)(cn.solid - cb.solid); w.dw[i] = (int64_t)(cn.v[0] - cb.v[0]);
    BudgetBasinRec& r = w.basins[label[i]];
    r.flags |= cb.fb | cn.fb | ((cn.ground != cn.ground || cb.ground != cb.ground) ? 4u : 0u);
    if (cn.ground < cb.ground) { r.lowered_cells++; if (-d > r.cut_max) { r.cut_max = -d; r.cut_cell = (uint32_t)i; } }
    if (cn.ground > cb.ground) { r.raised_cells++; if (d > r.fill_max) { r.fill_max = d; r.fill_cell = (uint32_t)i; } }
    if (cn.top != cb.top) {
      r.resurfaced_cells++;
      if (cn.top < ntypes) w.soils[cn.top].surfaced++;
      if (cb.top < ntypes) w.soils[cb.top].covered++;
    }
    if (cb.solid > cn.solid) add(r.eroded_q40, cb.solid - cn.solid, r.flags);
    if (cn.solid > cb.solid) add(r.deposited_q40, cn.solid - cb.solid, r.flags);
    if (cn.v[0] > cb.v[0]) add(r.water_gained_q40, cn.v[0] - cb.v[0], r.flags);
    if (cb.v[0] > cn.v[0]) add(r.water_lost_q40, cb.v[0] - cn.v[0], r.flags);
    for (uint32_t t = 0; t < ntypes && t < 71u; t++) {
      BudgetSoilRec& s = w.soils[t];
      s.flags |= cb.f[t] | cn.f[t];
      if (cn.v[t] > cb.v[t]) { add(s.gained_q40, cn.v[t] - cb.v[t], s.flags); s.cells_gained++; }
      if (cn.v[t] < cb.v[t]) { add(s.lost_q40, cb.v[t] - cn.v[t], s.flags); s.cells_lost++; }
      if (cn.x[t] > cb.x[t]) add(s.held_gained_q40, cn.x[t] - cb.x[t], s.flags);
      if (cn.x[t] < cb.x[t]) add(s.held_lost_q40, cb.x[t] - cn.x[t], s.flags);
    }
  }
  return w;
}
static bool same(const void* a, const void* b, size_t bytes) { return bytes == 0 || memcmp(a, b, bytes) == 0; }

static int check(int dx, int dy) {
  const Columns cb = columns(dx, dy);
  const Columns cn[3] = {changed(cb), changed(cb), changed(cb)};
  const size_t cells = (size_t)dx * dy;
  bh_map* base = host_map(cb, 1);
  bh_map* now[3] = {host_map(cn[0], 1), host_map(cn[1], 0), host_map(cn[2], 1)};
  int bad = 0;
  // the base's basins and labels, by the drainage host chain
  dh_map* chain[1] = {base};
  uint32_t nb = 0;
  std::vector<uint32_t> label(cells);
  dh_drainage(chain, 1, 0, 256, 0, 0, nullptr, &nb, nullptr, label.data(), nullptr);
  std::vector<BasinRec> drain(nb ? nb : 1);
  dh_drainage(chain, 1, 0, 256, 0, nb, drain.data(), &nb, nullptr, nullptr, nullptr);
  drain.resize(nb);
  const uint32_t NTS[2] = {64, 5};
  for (uint32_t nt : NTS) {
    Want want[3] = {restate(cb, cn[0], drain, label, nt), restate(cb, cn[1], drain, label, nt), restate(cb, cn[2], drain, label, nt)};
    for (int v = 0; v < bh_variants(); v++)
      for (uint32_t lanes : {64u, 256u})
        for (int order : {0, 3}) {
          // one pair, with the planes
          std::vector<BudgetBasinRec> out(nb ? nb : 1);
          std::vector<BudgetSoilRec> soils(nt);
          std::vector<double> dg(cells), dh(cells);
          std::vector<int64_t> ds(cells), dw(cells);
          uint32_t n = 0;
          uint64_t info[2] = {9, 9};
          bool ok = bh_budget(base, now, 1, v, lanes, order, nb, out.data(), sizeof(BudgetBasinRec), &n, soils.data(), sizeof(BudgetSoilRec), nt, dg.data(), dh.data(),
                              ds.data(), dw.data(), info) == 0 && n == nb;
          ok = ok && same(out.data(), want[0].basins.data(), nb * sizeof(BudgetBasinRec)) && same(soils.data(), want[0].soils.data(), nt * sizeof(BudgetSoilRec));
          ok = ok && same(dg.data(), want[0].dg.data(), cells * 8) && same(dh.data(), want[0].dh.data(), cells * 8) && same(ds.data(), want[0].ds.data(), cells * 8) &&
               same(dw.data(), want[0].dw.data(), cells * 8);
          // three members in one call, a cap one short of the count
          const uint32_t cap = nb > 1 ? nb - 1 : nb;
          std::vector<BudgetBasinRec> out3(3 * (size_t)cap + 1);
          std::vector<BudgetSoilRec> soils3(3 * (size_t)nt);
          ok = ok && bh_budget(base, now, 3, v, lanes, order, cap, out3.data(), sizeof(BudgetBasinRec), &n, soils3.data(), sizeof(BudgetSoilRec), nt, nullptr, nullptr,
                               nullptr, nullptr, info) == 0 && n == nb;
          for (int i = 0; ok && i < 3; i++)
            ok = same(out3.data() + (size_t)i * cap, want[i].basins.data(), cap * sizeof(BudgetBasinRec)) && same(soils3.data() + (size_t)i * nt, want[i].soils.data(), nt * sizeof(BudgetSoilRec));
          if (!ok) { printf("FAIL %dx%d ntypes %u variant %d lanes %u order %d\n", dx, dy, nt, v, lanes, order); bad++; }
        }
  }
  // corrupt chains: the deepest column of the base, then of member 1, gets a link out of the pool, then a cycle
  for (int which = 0; which < 2; which++) {
    const Columns& c = which == 0 ? cb : cn[1];
    bh_map* h = which == 0 ? base : now[1];
    size_t deep = 0;
    for (size_t i = 0; i < cells; i++) if (c.count[i] > c.count[deep]) deep = i;
    if (c.count[deep] < 3) continue;
    for (int kind = 0; kind < 2; kind++) {
      const uint32_t top = bh_prev(h, 0, deep, 0, 0), second = bh_prev(h, 1, top, 0, 0);
      bh_prev(h, 1, top, 1, kind == 0 ? (uint32_t)bh_pool_size(h) : top);   // (kind 1: the section under the top points at itself)
      BudgetBasinRec one;
      BudgetSoilRec soil;
      memset(&one, 0x5A, sizeof(one)); memset(&soil, 0x5A, sizeof(soil));
      const BudgetBasinRec keep = one;
      const BudgetSoilRec skeep = soil;
      uint32_t n = 7;
      uint64_t info[2] = {9, 9};
      const bool ok = bh_budget(base, now, 3, 0, 256, 0, 1, &one, 8, &n, &soil, 8, 1, nullptr, nullptr, nullptr, nullptr, info) == -5 &&
                      info[0] == (which == 0 ? 0u : 2u) && info[1] == deep && n == 7 && same(&one, &keep, sizeof(one)) && same(&soil, &skeep, sizeof(soil));
      bh_prev(h, 1, top, 1, second);
      if (!ok) { printf("FAIL %dx%d corrupt chain in map %d kind %d\n", dx, dy, which, kind); bad++; }
    }
  }
  for (bh_map* m : now) bh_destroy(m);
  bh_destroy(base);
  printf("%3dx%-3d %5u basins  %s\n", dx, dy, nb, bad ? "FAILED" : "ok");
  return bad;
}

int main() {
  int bad = 0;
  const int dims[4][2] = {{1, 1}, {5, 7}, {33, 47}, {96, 80}};
  for (const auto& d : dims) bad += check(d[0], d[1]);
  printf(bad ? "budget_check: FAILED\n" : "budget_check: OK\n");
  return bad ? 1 : 0;
}
