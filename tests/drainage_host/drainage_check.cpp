// drainage_check -- a stand-alone run of the drainage bodies for the sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o drainage_check drainage_check.cpp && ./drainage_check
// Without arguments: a cone, a ramp, a plateau, random heights and random heights under a Bernoulli(0.2) wet mask at 33 x 47 and
// 96 x 80, and three maps in one call, every tile shape, 64 and 256 lanes, the four launch orders, against plain loops in cell order
// (receiver, basin rank and area per cell; cells, wet cells and box per basin).
// With arguments: each names a dump written by tests/test_drainage_host.py -- an input of tests/drainage_ref.py (the cone, both ramps,
// the spiral trench, the plateau, the ties with -0.0 and the NaN cell, the random heights under the bernoulli20 and checker masks,
// corners, the empty columns; every size, 128 x 128 included) with the restatement's result: the columns' top records exactly as the
// snapshot holds them, then the count, the three planes and the records, all compared bit by bit. Every tile shape, 64 and 256 lanes,
// workgroups and lanes first to last and last to first. Little-endian words:
//   u32 magic 0x4E415244, i32 dimx, i32 dimy, u32 nsec, u32 count[cells], u32 type[nsec], f64 size[nsec], f64 floor[nsec],
//   u32 nbasins, u32 receivers[cells], u32 labels[cells], u32 area[cells], 48-byte records[nbasins]
// Exit status 0 = all equal.
#include "drainage_host.cpp"
#include "../analysis_host/analysis_check.h"

struct Want { std::vector<uint32_t> recv, label, area, cells, wetc, x0, y0, x1, y1; };
static Want plain(const Input& in) {
  const int dx = in.dx, dy = in.dy;
  const size_t n = in.h.size();
  auto height = [&](size_t c) { return in.wet[c] ? in.h[c] + 0.5 : in.h[c]; };
  Want w;
  w.recv.assign(n, DRAIN_NONE); w.label.assign(n, DRAIN_NONE); w.area.assign(n, 1u);
  // lakes by a flood fill in cell order: lake[c] = the smallest cell of c's lake
  std::vector<uint32_t> term(n, DRAIN_NONE), stack;
  for (uint32_t c0 = 0; c0 < n; c0++) {
    if (!in.wet[c0] || term[c0] != DRAIN_NONE) continue;
    term[c0] = c0; stack.push_back(c0);
    while (!stack.empty()) {
      const uint32_t c = stack.back(); stack.pop_back();
      for (int a = -1; a <= 1; a++) for (int b = -1; b <= 1; b++) {
        const int u = (int)(c / dy) + a, v = (int)(c % dy) + b;
        if ((a || b) && u >= 0 && v >= 0 && u < dx && v < dy && in.wet[(size_t)u * dy + v] && term[(size_t)u * dy + v] == DRAIN_NONE) {
          term[(size_t)u * dy + v] = c0; stack.push_back((uint32_t)(u * dy + v));
        }
      }
    }
  }
  for (uint32_t c = 0; c < n; c++) {
    if (in.wet[c]) continue;
    double best = height(c);
    for (int a = -1; a <= 1; a++) for (int b = -1; b <= 1; b++) {
      const int u = (int)(c / dy) + a, v = (int)(c % dy) + b;
      if ((a || b) && u >= 0 && v >= 0 && u < dx && v < dy && height((size_t)u * dy + v) < best) { best = height((size_t)u * dy + v); w.recv[c] = (uint32_t)(u * dy + v); }
    }
  }
  // donors before receivers: descending height (a receiver is strictly lower)
  std::vector<uint32_t> order(n);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return height(a) > height(b); });
  for (uint32_t c : order) if (w.recv[c] != DRAIN_NONE) w.area[w.recv[c]] += w.area[c];
  for (size_t i = n; i-- > 0;) {   // ascending height: the receiver's terminal is known
    const uint32_t c = order[i];
    if (in.wet[c]) continue;
    term[c] = w.recv[c] == DRAIN_NONE ? c : term[w.recv[c]];
  }
  std::vector<uint32_t> rank(n, DRAIN_NONE);
  uint32_t nb = 0;
  for (uint32_t c = 0; c < n; c++) if (term[c] == c) rank[c] = nb++;
  w.cells.assign(nb, 0); w.wetc.assign(nb, 0); w.x0.assign(nb, ~0u); w.y0.assign(nb, ~0u); w.x1.assign(nb, 0); w.y1.assign(nb, 0);
  for (uint32_t c = 0; c < n; c++) {
    const uint32_t r = rank[term[c]], x = c / dy, y = c % dy;
    w.label[c] = r; w.cells[r]++; w.wetc[r] += in.wet[c];
    w.x0[r] = std::min(w.x0[r], x); w.y0[r] = std::min(w.y0[r], y); w.x1[r] = std::max(w.x1[r], x); w.y1[r] = std::max(w.y1[r], y);
  }
  return w;
}

static int check(const char* name, const std::vector<Input>& ins) {
  std::vector<dh_map*> maps;
  std::vector<Want> wants;
  size_t words = 0;
  uint32_t cap = 0;
  for (const Input& in : ins) {
    maps.push_back(host_map(in)); wants.push_back(plain(in)); words += in.h.size();
    cap = std::max<uint32_t>(cap, (uint32_t)wants.back().cells.size() + 2u);
  }
  const uint32_t nm = (uint32_t)ins.size();
  int bad = 0;
  for (int v = 0; v < dh_variants(); v++)
    for (uint32_t lanes : {64u, 256u})
      for (int order = 0; order < 4; order++) {
        std::vector<uint32_t> nb(nm, 0), recv(words), label(words), area(words);
        std::vector<BasinRec> out((size_t)nm * cap);
        if (dh_drainage(maps.data(), nm, v, lanes, order, cap, out.data(), nb.data(), recv.data(), label.data(), area.data()) != 0) { bad++; continue; }
        bool ok = true;
        size_t at = 0;
        for (uint32_t i = 0; i < nm && ok; i++) {
          const Want& w = wants[i];
          const size_t n = w.recv.size();
          ok = nb[i] == w.cells.size() && std::equal(w.recv.begin(), w.recv.end(), recv.begin() + at) && std::equal(w.label.begin(), w.label.end(), label.begin() + at) &&
               std::equal(w.area.begin(), w.area.end(), area.begin() + at);
          for (uint32_t r = 0; ok && r < nb[i]; r++) {
            const BasinRec& b = out[(size_t)i * cap + r];
            ok = b.cells == w.cells[r] && b.wet_cells == w.wetc[r] && b.x0 == w.x0[r] && b.y0 == w.y0[r] && b.x1 == w.x1[r] && b.y1 == w.y1[r] &&
                 w.label[b.first_cell] == r && ((b.flags & 1u) != 0) == (w.wetc[r] != 0) && b.flags <= 3u && b.reserved[0] == 0u && b.reserved[1] == 0u;
          }
          at += n;
        }
        if (!ok) { printf("FAIL %s variant %d lanes %u order %d\n", name, v, lanes, order); bad++; }
      }
  for (dh_map* m : maps) dh_destroy(m);
  printf("%-10s %zu map(s), %5zu basins in the first  %s\n", name, ins.size(), wants[0].cells.size(), bad ? "FAILED" : "ok");
  return bad;
}

static int check_dump(const char* path) {
  Columns in;
  uint32_t nb = 0;
  std::vector<uint32_t> recv, label, area;
  std::vector<BasinRec> recs;
  if (!read_dump(path, 0x4E415244u, in, [&](FILE* f) {
        return fread(&nb, 4, 1, f) == 1 && nb <= in.cells && take(f, recv, in.cells) && take(f, label, in.cells) && take(f, area, in.cells) && take(f, recs, nb);
      })) return 1;
  const size_t n = in.cells;
  dh_map* h = in.map();
  int bad = 0;
  for (int v = 0; v < dh_variants(); v++)
    for (uint32_t lanes : {64u, 256u})
      for (int order : {0, 3}) {
        uint32_t got = 0;
        std::vector<uint32_t> r(n), l(n), a(n);
        std::vector<BasinRec> out((size_t)nb + 2u);
        memset(out.data(), 0, out.size() * sizeof(BasinRec));
        const bool same = dh_drainage(&h, 1, v, lanes, order, nb + 2u, out.data(), &got, r.data(), l.data(), a.data()) == 0 && got == nb && r == recv && l == label &&
                          a == area && (nb == 0 || memcmp(out.data(), recs.data(), (size_t)nb * sizeof(BasinRec)) == 0);
        if (!same) { printf("FAIL %s variant %d lanes %u order %d: %u basins, expected %u\n", path, v, lanes, order, got, nb); bad++; }
      }
  dh_destroy(h);
  printf("%-32s %4ux%-4u %6u basins  %s\n", file_name(path), in.dimx, in.dimy, nb, bad ? "FAILED" : "ok");
  return bad;
}

int main(int argc, char** argv) {
  return check_main(argc, argv, check_dump, {"cone", "ramp", "plateau", "random", "lakes"}, {{"lakes", 33, 47}, {"cone", 70, 1}, {"random", 1, 70}},
                    [](const char* name, const std::vector<MapSpec>& specs) { return check(name, make_all(specs)); });
}
