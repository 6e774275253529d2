// Host-only test of the output side of the host layer: the table of the mesh's rows (kRows) and the table of the optional
// outputs (kAttrWords).  The list of device buffers, the emit's and the keep's reservation sizes against the formulas written
// out per row, every refusal of an attribute against its full text, and the rows' way home before a count.  No device is
// touched: the program includes the host layer and never creates a context through the ABI.  Built plain for the suite
// (tests/test_row_table.py); the same source under -Xarch_host -fsanitize=address,undefined is the sanitizer run of this code.
#include "../cuberille_api.hip"

#include <cstdio>
#include <set>

namespace {

int failures = 0;
#define EXPECT(cond, ...)                                                    \
  do {                                                                       \
    if (!(cond)) {                                                           \
      failures++;                                                            \
      std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond);        \
      std::printf(__VA_ARGS__);                                              \
      std::printf("\n");                                                     \
    }                                                                        \
  } while (0)

void buffer_list() {
  cuberille_ctx c;
  const std::vector<DevBuf *> all = device_buffers(&c);
  const std::set<DevBuf *> distinct(all.begin(), all.end());
  EXPECT(all.size() == 38 && distinct.size() == 38, "%zu buffers, %zu distinct", all.size(), distinct.size());
  auto once = [&](DevBuf *b, const char *what, int r) {
    EXPECT(std::count(all.begin(), all.end(), b) == 1, "%s %d is listed %d times", what, r, (int)std::count(all.begin(), all.end(), b));
  };
  for (int r = 0; r < N_ROWS; r++) {
    once(&c.rows[r].row, "row", r);
    once(&c.rows[r].spare, "spare", r);
  }
  DevBuf *const scratch[4] = {&c.compParent, &c.compScan, &c.keepSel, &c.keepScan};
  for (int i = 0; i < 4; i++) once(scratch[i], "scratch", i);
  // ... which the context lists once, as the components' scratch
  EXPECT(std::set<DevBuf *>(c.compScratch, c.compScratch + 4) == std::set<DevBuf *>(scratch, scratch + 4), "the components' scratch");
}

bool same(const Want &a, const Want &b) { return a.bytes == b.bytes && a.cover == b.cover; }

// emit_sizes against the sizes written out row by row, none of them through the table
void emit_reservations() {
  const Grid g{};
  const Tuning t{};
  const u64 counts[5] = {0, 1, 63, 64, 65};
  const size_t pixels[4] = {1, 2, 4, 8};
  int cases = 0;
  for (u64 nV : counts)
    for (u64 nQ = 0; nQ < 2; nQ++)
      for (u64 ghostQ = 0; ghostQ < 2; ghostQ++)                 // totQ >= nQ: quads of the ghost slice ahead of the owned ones
        for (int triangles = 0; triangles < 2; triangles++)
          for (int dyn = 0; dyn < 2; dyn++)
            for (size_t planeCorners : {(size_t)0, (size_t)35})
              for (int set = 0; set < 8; set++)
                for (size_t pixel : pixels) {
                  const bool normals = set & 1, cellPixels = set & 2, components = set & 4;
                  const u64 totQ = nQ + ghostQ;
                  const bool on[N_ATTRS] = {normals, cellPixels, components};
                  const EmitSizes s = emit_sizes(g, t, triangles, dyn, nV, totQ, nQ, planeCorners, 1000, on, pixel);
                  const u64 nextV = dyn ? nV : nV + nV / 4 + 4096, nextQ = dyn ? nQ : totQ + totQ / 4 + 4096;
                  const size_t quad = (triangles ? 6 : 4) * sizeof(u64);
                  const size_t perQuad = (triangles ? 2 : 1) * (cellPixels ? pixel : 0);
                  const u64 nC = nQ * (triangles ? 2 : 1), nextC = nextQ * (triangles ? 2 : 1);
                  const bool comp = components && nV;
                  const Want none{0, 0};
                  Want want[N_ROWS];
                  want[ROW_POINTS] = {(size_t)(nV + planeCorners ? nV + planeCorners : 1) * 3 * sizeof(float), (size_t)(nextV + planeCorners) * 3 * sizeof(float)};
                  want[ROW_CELLS] = {(size_t)(nQ ? nQ : 1) * quad, (size_t)nextQ * quad};
                  want[ROW_NORMALS] = normals && nV ? Want{(size_t)nV * 3 * sizeof(float), (size_t)nextV * 3 * sizeof(float)} : none;
                  want[ROW_CELL_PIX] = perQuad && nQ ? Want{(size_t)nQ * perQuad, (size_t)nextQ * perQuad} : none;
                  want[ROW_COMP_POINT] = comp ? Want{(size_t)nV * sizeof(u32), (size_t)nextV * sizeof(u32)} : none;
                  want[ROW_COMP_CELL] = comp ? Want{(size_t)(nC ? nC : 1) * sizeof(u32), (size_t)nextC * sizeof(u32)} : none;
                  want[ROW_COMP_COUNT] = comp ? Want{(size_t)nV * sizeof(u64), (size_t)nextV * sizeof(u64)} : none;
                  const Want scan = components ? Want{comp_scan_bytes(nV), comp_scan_bytes(nextV)} : none;
                  for (int r = 0; r < N_ROWS; r++)
                    EXPECT(same(s.rows[r], want[r]), "%s: nV %llu nQ %llu totQ %llu triangles %d dyn %d plane %zu set %d pixel %zu: %zu / %zu, expected %zu / %zu",
                           kRows[r].name, (unsigned long long)nV, (unsigned long long)nQ, (unsigned long long)totQ, triangles, dyn, planeCorners, set, pixel,
                           s.rows[r].bytes, s.rows[r].cover, want[r].bytes, want[r].cover);
                  EXPECT(same(s.compScan, scan), "compScan: nV %llu set %d: %zu / %zu", (unsigned long long)nV, set, s.compScan.bytes, s.compScan.cover);
                  cases++;
                }
  EXPECT(cases == 5 * 2 * 2 * 2 * 2 * 2 * 8 * 4, "%d cases", cases);
  // the three the table could get wrong most easily, by their figures
  const bool all[N_ATTRS] = {true, true, true};
  const EmitSizes empty = emit_sizes(g, t, true, false, 0, 0, 0, 0, 1000, all, 2);
  EXPECT(empty.rows[ROW_NORMALS].bytes == 0, "no point: no normals");
  EXPECT(empty.compScan.bytes == comp_scan_bytes(0) && empty.compScan.bytes >= sizeof(u64), "K's slot also for an empty mesh");
  EXPECT(!empty.rows[ROW_COMP_POINT].bytes && !empty.rows[ROW_COMP_CELL].bytes && !empty.rows[ROW_COMP_COUNT].bytes, "no point: no component rows");
  EXPECT(empty.rows[ROW_CELLS].bytes == 48 && empty.rows[ROW_POINTS].bytes == 12, "an empty mesh: one quad of two triangles, one point");
  const EmitSizes one = emit_sizes(g, t, true, true, 1, 1, 1, 0, 1000, all, 2);
  EXPECT(one.rows[ROW_CELL_PIX].bytes == 4 && one.rows[ROW_CELL_PIX].cover == 4, "two cells per quad with triangles, two bytes each");
}

// the spare rows of cuberille_keep_components, by the kept counts
void keep_reservations() {
  for (u64 nP2 : {(u64)1, (u64)65})
    for (u64 nC2 : {(u64)0, (u64)1, (u64)64})
      for (u64 K2 : {(u64)1, (u64)3})
        for (int nv = 3; nv <= 4; nv++)
          for (size_t pix : {(size_t)1, (size_t)8}) {
            const u64 n2[N_PERS] = {nP2, nC2, K2};
            const size_t want[N_ROWS] = {(size_t)nP2 * 3 * sizeof(float), (size_t)(nC2 ? nC2 : 1) * nv * sizeof(u64), (size_t)nP2 * 3 * sizeof(float),
                                         (size_t)(nC2 ? nC2 : 1) * pix, (size_t)nP2 * sizeof(u32), (size_t)(nC2 ? nC2 : 1) * sizeof(u32),
                                         (size_t)K2 * sizeof(u64)};
            for (int r = 0; r < N_ROWS; r++)
              EXPECT(row_reserve_bytes(r, n2, nv, pix) == want[r], "spare %s: %zu, expected %zu", kRows[r].name, row_reserve_bytes(r, n2, nv, pix), want[r]);
          }
}

// every refusal in full; {0} stands for the attribute's words
const char *const kNoun[N_ATTRS] = {"point normals", "cell pixels", "components"};
const char *const kFn[N_ATTRS] = {"cuberille_set_point_normals", "cuberille_set_cell_pixels", "cuberille_set_components"};
enum Outcome { OFFERED, NO_STEP, NO_GROUP, NO_SLAB };
const char *const kText[N_ATTRS][4] = {
    {nullptr, "point normals (cuberille_set_point_normals) belong to one context's whole volume: not offered with the cuberille_step_* calls",
     "has point normals set (cuberille_set_point_normals): they belong to one context's whole volume, not offered in a group",
     "point normals (cuberille_set_point_normals) belong to a whole volume: not offered on slabs"},
    {nullptr, "cell pixels (cuberille_set_cell_pixels) belong to one context's whole volume: not offered with the cuberille_step_* calls",
     "has cell pixels set (cuberille_set_cell_pixels): they belong to one context's whole volume, not offered in a group",
     "cell pixels (cuberille_set_cell_pixels) belong to a whole volume: not offered on slabs"},
    {nullptr, "components (cuberille_set_components) belong to one context's whole volume: not offered with the cuberille_step_* calls",
     "has components set (cuberille_set_components): they belong to one context's whole volume, not offered in a group",
     "components (cuberille_set_components) belong to a whole volume: not offered on slabs"},
};
const char *const kHeld = "point normals (cuberille_set_point_normals) are not offered on a context holding a gradient "
                          "(cuberille_hold_gradient): the reference would evaluate the stale image there";
const char *const kGaussian = "point normals (cuberille_set_point_normals) are the central-difference gradient: not offered with "
                              "CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN";
// [route][the whole volume, an explicit slab that is the whole buffer, a true slab], the same for the three attributes: the
// route's refusal comes first (validate, the group's loop), a slab's behind it (count_prepare)
const Outcome kOutcome[N_ROUTES][3] = {
    {OFFERED, OFFERED, NO_SLAB},      // ROUTE_DEVICE
    {OFFERED, OFFERED, NO_SLAB},      // ROUTE_HOST
    {OFFERED, OFFERED, NO_SLAB},      // ROUTE_SLAB
    {NO_STEP, NO_STEP, NO_STEP},      // ROUTE_STEP
    {OFFERED, OFFERED, NO_SLAB},      // ROUTE_STREAM
    {NO_GROUP, NO_GROUP, NO_GROUP},   // ROUTE_GROUP
    {OFFERED, OFFERED, NO_SLAB},      // ROUTE_WARM_UP
};

void names_only(const char *why, int a, const char *what) {
  for (int k = 0; k < N_ATTRS; k++) {
    const bool word = std::strstr(why, kNoun[k]) != nullptr, fn = std::strstr(why, kFn[k]) != nullptr;
    if (k == a) EXPECT(word && fn, "%s: \"%s\" should name the %s", what, why, kNoun[k]);
    else EXPECT(!word && !fn, "%s: \"%s\" should not name the %s", what, why, kNoun[k]);
  }
}

void refusals() {
  const int64_t nz = 10;
  const cuberille_slab slabs[3] = {{}, {nz, 0, 0, nz, 0, 0, nullptr, nullptr}, {40, 10, 12, 18, 0, 0, nullptr, nullptr}};
  cuberille_params prm{};
  for (int a = 0; a < N_ATTRS; a++)
    for (int route = 0; route < N_ROUTES; route++)
      for (int k = 0; k < 3; k++)
        for (int feature = 0; feature < 3; feature++) {          // 0 none, 1 a held gradient, 2 the recursive-Gaussian gradient
          cuberille_ctx c;
          c.attr[a].on = true;
          c.holdGradient = feature == 1;
          prm.gradient_variant = feature == 2 ? CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN : CUBERILLE_GRADIENT_CENTRAL;
          const char *why = nullptr;
          const int rc = attrs_offered(&c, &prm, (Route)route, k ? &slabs[k] : nullptr, nz, &why);
          char what[96];
          std::snprintf(what, sizeof what, "attribute %d route %d slab %d feature %d", a, route, k, feature);
          // (the normals' own two come behind the route's refusal and ahead of the slab's, as validate runs ahead of count_prepare)
          const char *expect = kText[a][kOutcome[route][k]];
          if (a == ATTR_NORMALS && feature && kOutcome[route][k] != NO_STEP && kOutcome[route][k] != NO_GROUP) expect = feature == 1 ? kHeld : kGaussian;
          if (!expect) {
            EXPECT(rc == CUBERILLE_OK && why && !*why, "%s: rc %d \"%s\"", what, rc, why ? why : "(null)");
          } else {
            EXPECT(rc == CUBERILLE_ERR_ARGUMENT && why && !std::strcmp(why, expect), "%s: rc %d \"%s\", expected \"%s\"", what, rc, why ? why : "(null)", expect);
            if (why) names_only(why, a, what);
          }
        }
  // an all-zero slab is the whole volume
  cuberille_ctx c;
  c.attr[ATTR_COMPONENTS].on = true;
  const char *why = nullptr;
  EXPECT(attrs_offered(&c, &prm, ROUTE_SLAB, &slabs[0], nz, &why) == CUBERILLE_OK, "an all-zero slab");
  // count_prepare asks about the slab alone (no parameters): the normals' own two refusals are validate's
  cuberille_ctx held;
  held.attr[ATTR_NORMALS].on = held.holdGradient = true;
  EXPECT(attrs_offered(&held, nullptr, ROUTE_SLAB, &slabs[1], nz, &why) == CUBERILLE_OK, "a slab that is the whole buffer: \"%s\"", why);
  EXPECT(attrs_offered(&held, nullptr, ROUTE_SLAB, &slabs[2], nz, &why) == CUBERILLE_ERR_ARGUMENT && !std::strcmp(why, kText[ATTR_NORMALS][NO_SLAB]), "\"%s\"", why);
  // the state error of each; of two attributes that are on, the first one's refusal
  const char *const missing[N_ATTRS] = {"no point normals: the last extraction ran with the setting off (cuberille_set_point_normals)",
                                        "no cell pixels: the last extraction ran with the setting off (cuberille_set_cell_pixels)",
                                        "no components: the last extraction ran with the setting off (cuberille_set_components)"};
  for (int a = 0; a < N_ATTRS; a++) {
    cuberille_ctx m;
    EXPECT(attr_preconditions(&m, a) == CUBERILLE_ERR_STATE && m.err == "no mesh: call cuberille_extract_* or cuberille_emit first", "\"%s\"", m.err.c_str());
    m.haveMesh = true;
    EXPECT(attr_preconditions(&m, a) == CUBERILLE_ERR_STATE && m.err == missing[a], "\"%s\"", m.err.c_str());
    m.attr[a].have = true;
    EXPECT(attr_preconditions(&m, a) == CUBERILLE_OK, "attribute %d at hand", a);
  }
  prm.gradient_variant = CUBERILLE_GRADIENT_CENTRAL;
  cuberille_ctx two;
  two.attr[ATTR_CELL_PIXELS].on = two.attr[ATTR_COMPONENTS].on = true;
  EXPECT(attrs_offered(&two, &prm, ROUTE_STEP, nullptr, 0, &why) == CUBERILLE_ERR_ARGUMENT && !std::strcmp(why, kText[ATTR_CELL_PIXELS][NO_STEP]), "\"%s\"", why);
  EXPECT(attrs_offered(&two, &prm, ROUTE_DEVICE, nullptr, 0, &why) == CUBERILLE_OK, "both offered on a whole volume");
  cuberille_ctx none;
  EXPECT(attrs_offered(&none, &prm, ROUTE_STEP, &slabs[2], nz, &why) == CUBERILLE_OK, "nothing on: nothing refused");
}

// rows_home on a bare context: capacities set by hand, no memory behind them (p stays null: nothing is ever freed)
void rows_go_home() {
  for (int set = 0; set < 8; set++) {
    cuberille_ctx c;
    for (int a = 0; a < N_ATTRS; a++) c.attr[a].on = (set >> a) & 1;
    for (int r = 0; r < N_ROWS; r++) { c.rows[r].row.cap = 100 + r; c.rows[r].spare.cap = 1000 + r; }
    for (int pass = 0; pass < 2; pass++) {                     // (the second time they are at home already: nothing moves)
      rows_home(&c);
      for (int r = 0; r < N_ROWS; r++) {
        // (the mesh's own rows and the components' always; the normals and the cell pixels while their setting is on)
        const bool moves = r == ROW_NORMALS ? c.attr[ATTR_NORMALS].on : r == ROW_CELL_PIX ? c.attr[ATTR_CELL_PIXELS].on : true;
        EXPECT(c.rows[r].row.cap == (moves ? 1000u + r : 100u + r) && c.rows[r].spare.cap == (moves ? 100u + r : 1000u + r),
               "set %d pass %d, %s: row %zu spare %zu", set, pass, kRows[r].name, c.rows[r].row.cap, c.rows[r].spare.cap);
        EXPECT(!c.rows[r].row.p && !c.rows[r].spare.p, "no memory");
      }
    }
  }
  // the larger one already in its place, and equal ones: as they are
  cuberille_ctx c;
  for (int a = 0; a < N_ATTRS; a++) c.attr[a].on = true;
  for (int r = 0; r < N_ROWS; r++) { c.rows[r].row.cap = 500; c.rows[r].spare.cap = r % 2 ? 500 : 20 + r; }
  rows_home(&c);
  for (int r = 0; r < N_ROWS; r++) EXPECT(c.rows[r].row.cap == 500 && c.rows[r].spare.cap == (r % 2 ? 500u : 20u + r), "%s stays", kRows[r].name);
  // a setting that goes off and on with nothing reserved touches no device and only moves its flag
  for (int a = 0; a < N_ATTRS; a++) {
    cuberille_ctx s;
    EXPECT(set_attr(&s, a, 1) == CUBERILLE_OK && s.attr[a].on && !s.attr[a].counting && !s.attr[a].have, "attribute %d on", a);
    bool released = false;
    EXPECT(set_attr(&s, a, 0, &released) == CUBERILLE_OK && !s.attr[a].on && !released, "attribute %d off", a);
    s.stepMode = 1;
    EXPECT(set_attr(&s, a, 1) == CUBERILLE_ERR_STATE && !s.attr[a].on && s.err == "a step is open on this context", "attribute %d, a step open", a);
  }
}

}  // namespace

int main() {
  buffer_list();
  emit_reservations();
  keep_reservations();
  refusals();
  rows_go_home();
  std::printf(failures ? "row_table: %d check(s) FAILED\n" : "row_table ok\n", failures);
  return failures ? 1 : 0;
}
