// lakes_check -- a stand-alone run of the census bodies for the sanitizers (not part of the pytest suite):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o lakes_check lakes_check.cpp && ./lakes_check
// The spiral, the comb and a Bernoulli(0.41) mask at 33 x 47 and 96 x 80, every tile shape, 64 and 256 lanes, both launch orders,
// against a flood fill in cell order (lake count, label plane, cells and box per lake). Exit status 0 = all equal.
#include <cstdio>
#include <cstdlib>

#include "lakes_host.cpp"

static std::vector<uint8_t> spiral(int dx, int dy) {
  std::vector<uint8_t> m((size_t)dx * dy, 0);
  const int dir[4][2] = {{0, 1}, {1, 0}, {0, -1}, {-1, 0}};
  auto in = [&](int u, int v) { return u >= 0 && v >= 0 && u < dx && v < dy; };
  int x = 0, y = 0, d = 0;
  m[0] = 1;
  for (;;) {
    int turn = 0;
    for (; turn < 2; turn++) {
      const int* k = dir[(d + turn) % 4];
      const int u = x + k[0], v = y + k[1], u2 = x + 2 * k[0], v2 = y + 2 * k[1];
      if (in(u, v) && !m[(size_t)u * dy + v] && !(in(u2, v2) && m[(size_t)u2 * dy + v2])) { d = (d + turn) % 4; x = u; y = v; m[(size_t)x * dy + y] = 1; break; }
    }
    if (turn == 2) return m;
  }
}
static std::vector<uint8_t> comb(int dx, int dy) {
  std::vector<uint8_t> m((size_t)dx * dy, 0);
  for (int x = 0; x < dx; x++) for (int y = 0; y < dy; y++) m[(size_t)x * dy + y] = (y % 2 == 0 || x == dx - 1) ? 1 : 0;
  return m;
}
static std::vector<uint8_t> bernoulli(int dx, int dy, double p) {
  std::vector<uint8_t> m((size_t)dx * dy, 0);
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (auto& c : m) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; c = (double)(s >> 11) * (1.0 / 9007199254740992.0) < p ? 1 : 0; }
  return m;
}

struct Want { std::vector<uint32_t> label, cells, x0, y0, x1, y1; };
static Want flood(const std::vector<uint8_t>& m, int dx, int dy) {
  Want w;
  w.label.assign(m.size(), LAKE_DRY);
  std::vector<uint32_t> stack;
  for (uint32_t c0 = 0; c0 < m.size(); c0++) {
    if (!m[c0] || w.label[c0] != LAKE_DRY) continue;
    const uint32_t r = (uint32_t)w.cells.size();
    w.cells.push_back(0); w.x0.push_back(~0u); w.y0.push_back(~0u); w.x1.push_back(0); w.y1.push_back(0);
    w.label[c0] = r; stack.push_back(c0);
    while (!stack.empty()) {
      const uint32_t c = stack.back(); stack.pop_back();
      const uint32_t x = c / dy, y = c % dy;
      w.cells[r]++;
      if (x < w.x0[r]) w.x0[r] = x; if (y < w.y0[r]) w.y0[r] = y; if (x > w.x1[r]) w.x1[r] = x; if (y > w.y1[r]) w.y1[r] = y;
      for (int a = -1; a <= 1; a++) for (int b = -1; b <= 1; b++) {
        const int u = (int)x + a, v = (int)y + b;
        if ((a || b) && u >= 0 && v >= 0 && u < dx && v < dy && m[(size_t)u * dy + v] && w.label[(size_t)u * dy + v] == LAKE_DRY) {
          w.label[(size_t)u * dy + v] = r; stack.push_back((uint32_t)(u * dy + v));
        }
      }
    }
  }
  return w;
}

static int check(const char* name, const std::vector<uint8_t>& m, int dx, int dy) {
  const size_t n = m.size();
  std::vector<uint32_t> count(n), type, plane(n);
  std::vector<double> size, floor;
  for (size_t c = 0; c < n; c++) {
    count[c] = m[c] ? 2 : 1;
    type.push_back(1); size.push_back(1.0 + 0.125 * (double)(c % 5)); floor.push_back(0.0);
    if (m[c]) { type.push_back(0); size.push_back(0.5); floor.push_back(size[size.size() - 2]); }
  }
  lh_map* h = lh_create(dx, dy, count.data(), type.data(), size.data(), floor.data());
  const Want w = flood(m, dx, dy);
  int bad = 0;
  for (int v = 0; v < lh_variants(); v++)
    for (uint32_t lanes : {64u, 256u})
      for (int desc = 0; desc < 2; desc++) {
        uint32_t nl = 0;
        const uint32_t cap = (uint32_t)w.cells.size() + 2u;
        std::vector<LakeRec> out(cap);
        if (lh_census(&h, 1, v, lanes, desc, cap, out.data(), &nl, plane.data()) != 0) { bad++; continue; }
        bool ok = nl == w.cells.size() && plane == w.label;
        for (uint32_t r = 0; ok && r < nl; r++)
          ok = out[r].cells == w.cells[r] && out[r].x0 == w.x0[r] && out[r].y0 == w.y0[r] && out[r].x1 == w.x1[r] && out[r].y1 == w.y1[r] &&
               out[r].volume_q40 == (uint64_t)w.cells[r] << 39 && out[r].flags <= 1u;
        if (!ok) { printf("FAIL %s %dx%d variant %d lanes %u descending %d: %u lakes, expected %zu\n", name, dx, dy, v, lanes, desc, nl, w.cells.size()); bad++; }
      }
  lh_destroy(h);
  printf("%-10s %3dx%-3d %5zu lakes  %s\n", name, dx, dy, w.cells.size(), bad ? "FAILED" : "ok");
  return bad;
}

int main() {
  int bad = 0;
  const int dims[2][2] = {{33, 47}, {96, 80}};
  for (const auto& d : dims) {
    bad += check("spiral", spiral(d[0], d[1]), d[0], d[1]);
    bad += check("comb", comb(d[0], d[1]), d[0], d[1]);
    bad += check("random41", bernoulli(d[0], d[1], 0.41), d[0], d[1]);
  }
  return bad ? 1 : 0;
}
