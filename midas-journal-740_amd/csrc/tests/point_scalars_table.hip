// Host-only test of the point scalars' row (cuberille_set_point_scalars), the optional output the host layer holds BESIDE its
// tables: the row's and the spare's reservation sizes against 8 * n written out, every refusal's words per route,
// the state error's text, what the setter refuses without touching a device, and that a bare context's rows_home leaves the new
// pair alone while the setting is off.  No device is touched: the program includes the host layer and never creates a context
// through the ABI.  Built plain and under -Xarch_host -fsanitize=address,undefined (tests/test_point_scalars.py).
#include "../cuberille_api.hip"

#include <cstdio>

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

void reservations() {
  const u64 counts[6] = {0, 1, 255, 256, 257, (1ull << 32) + 1};
  for (u64 n : counts) {
    const Want w = point_scalars_want(n);
    const size_t bytes = n ? (size_t)(8 * n) : 0, cover = n ? (size_t)(8 * (n + n / 4 + 4096)) : 0;
    EXPECT(w.bytes == bytes && w.cover == cover, "the row of %llu points: %zu / %zu, expected %zu / %zu", (unsigned long long)n, w.bytes, w.cover, bytes, cover);
    const Want d = point_scalars_want(n, true);
    EXPECT(d.bytes == bytes && d.cover == bytes, "the row of a blind launch sized for %llu points: %zu / %zu", (unsigned long long)n, d.bytes, d.cover);
    EXPECT(point_scalars_bytes(n) == (size_t)(8 * n), "the spare of a keep to %llu points: %zu", (unsigned long long)n, point_scalars_bytes(n));
  }
  EXPECT(point_scalars_want((1ull << 32) + 1).bytes == 34359738376ull, "2^32 + 1 points by its figure");
}

void buffers() {
  cuberille_ctx c;
  const size_t bare = device_buffers(&c).size();
  c.ps.on = true;
  const std::vector<DevBuf *> all = device_buffers(&c);
  EXPECT(all.size() == bare + 3, "%zu buffers with the setting on, %zu off", all.size(), bare);
  for (DevBuf *b : {&c.ps.rows.row, &c.ps.rows.spare, &c.ps.copy})
    EXPECT(std::count(all.begin(), all.end(), b) == 1, "a buffer of the point scalars is listed %d times", (int)std::count(all.begin(), all.end(), b));
}

const char *const kStep = "point scalars (cuberille_set_point_scalars) belong to one context's whole volume: not offered with the cuberille_step_* calls";
const char *const kGroup = "has point scalars set (cuberille_set_point_scalars): they belong to one context's whole volume, not offered in a group";
const char *const kSlab = "point scalars (cuberille_set_point_scalars) belong to a whole volume: not offered on slabs";

void refusals() {
  const int64_t nz = 10;
  const cuberille_slab slabs[3] = {{}, {nz, 0, 0, nz, 0, 0, nullptr, nullptr}, {40, 10, 12, 18, 0, 0, nullptr, nullptr}};
  cuberille_params prm{};
  for (int route = 0; route < N_ROUTES; route++)
    for (int k = 0; k < 3; k++)
      for (int feature = 0; feature < 3; feature++) {            // 0 none, 1 a held gradient, 2 the recursive-Gaussian gradient: both offered
        cuberille_ctx c;
        c.ps.on = true;
        c.holdGradient = feature == 1;
        prm.gradient_variant = feature == 2 ? CUBERILLE_GRADIENT_RECURSIVE_GAUSSIAN : CUBERILLE_GRADIENT_CENTRAL;
        const char *why = nullptr;
        const int rc = attrs_offered(&c, &prm, (Route)route, k ? &slabs[k] : nullptr, nz, &why);
        const char *expect = route == ROUTE_STEP ? kStep : route == ROUTE_GROUP ? kGroup : k == 2 ? kSlab : nullptr;
        if (!expect) EXPECT(rc == CUBERILLE_OK && why && !*why, "route %d slab %d: rc %d \"%s\"", route, k, rc, why ? why : "(null)");
        else EXPECT(rc == CUBERILLE_ERR_ARGUMENT && why && !std::strcmp(why, expect), "route %d slab %d: rc %d \"%s\", expected \"%s\"", route, k, rc, why ? why : "(null)", expect);
      }
  // behind the tables' attributes: of two that are on, the table's refusal comes first
  cuberille_ctx two;
  two.ps.on = two.attr[ATTR_COMPONENTS].on = true;
  const char *why = nullptr;
  EXPECT(attrs_offered(&two, &prm, ROUTE_STEP, nullptr, 0, &why) == CUBERILLE_ERR_ARGUMENT && std::strstr(why, "components") && !std::strstr(why, "point scalars"), "\"%s\"", why);
  cuberille_ctx none;
  EXPECT(attrs_offered(&none, &prm, ROUTE_STEP, &slabs[2], nz, &why) == CUBERILLE_OK, "nothing on: nothing refused");
  // the state error
  cuberille_ctx m;
  EXPECT(point_scalars_preconditions(&m) == CUBERILLE_ERR_STATE && m.err == "no mesh: call cuberille_extract_* or cuberille_emit first", "\"%s\"", m.err.c_str());
  m.haveMesh = true;
  EXPECT(point_scalars_preconditions(&m) == CUBERILLE_ERR_STATE &&
             m.err == "no point scalars: the last extraction ran with the setting off (cuberille_set_point_scalars)", "\"%s\"", m.err.c_str());
  const double *d = (const double *)&m;
  EXPECT(cuberille_point_scalars_device(&m, &d) == CUBERILLE_ERR_STATE && d == nullptr, "the getter's state error");
  m.ps.have = true;
  EXPECT(point_scalars_preconditions(&m) == CUBERILLE_OK, "the row at hand");
  EXPECT(cuberille_point_scalars_device(&m, &d) == CUBERILLE_OK && d == nullptr, "an empty mesh: a null pointer");
  EXPECT(cuberille_point_scalars_download(&m, nullptr, 0) == CUBERILLE_OK, "an empty mesh: an empty download");
  m.res.n_points = 3;
  EXPECT(cuberille_point_scalars_download(&m, nullptr, 23) == CUBERILLE_ERR_ARGUMENT && m.err == "the point scalars take 24 bytes, the buffer holds 23", "\"%s\"", m.err.c_str());
}

// what the setter says without a device: every refusal names the setting, and leaves it as it was
void setter() {
  cuberille_image_desc d{};
  d.pixel_type = CUBERILLE_PIX_F32;
  for (int i = 0; i < 3; i++) { d.dims[i] = 4; d.spacing[i] = 1.0; d.direction[4 * i] = 1.0; }
  float vox[64] = {};
  auto refused = [&](const cuberille_image_desc &desc, const void *v, int location, const char *what) {
    cuberille_ctx c;
    const int rc = cuberille_set_point_scalars(&c, &desc, v, location, 0.0);
    EXPECT(rc == CUBERILLE_ERR_ARGUMENT && c.err.find("point scalars") != std::string::npos && !c.ps.on, "%s: rc %d \"%s\"", what, rc, c.err.c_str());
  };
  refused(d, nullptr, CUBERILLE_MEM_HOST, "a null pointer");
  refused(d, vox, 2, "an unknown location");
  refused(d, vox, -1, "a negative location");
  cuberille_image_desc bad = d;
  bad.pixel_type = 99;
  refused(bad, vox, CUBERILLE_MEM_DEVICE, "an unknown pixel type");
  bad = d; bad.dims[1] = 0;
  refused(bad, vox, CUBERILLE_MEM_DEVICE, "an empty axis");
  bad = d; bad.dims[2] = 0x80000000LL;
  refused(bad, vox, CUBERILLE_MEM_DEVICE, "an axis past 2^31 - 1");
  bad = d; bad.spacing[0] = 0.0;
  refused(bad, vox, CUBERILLE_MEM_DEVICE, "a zero spacing");
  bad = d; bad.spacing[2] = -1.0;
  refused(bad, vox, CUBERILLE_MEM_DEVICE, "a negative spacing");
  bad = d; bad.index_start[0] = (1LL << 30) + 1;
  refused(bad, vox, CUBERILLE_MEM_DEVICE, "a start index past 2^30");
  bad = d; bad.direction[0] = 0.0;
  refused(bad, vox, CUBERILLE_MEM_DEVICE, "a singular direction");
  // a borrowed device pointer touches no device: the setting as given, then off again
  cuberille_ctx c;
  EXPECT(cuberille_set_point_scalars(&c, &d, vox, CUBERILLE_MEM_DEVICE, -0.0) == CUBERILLE_OK && c.ps.on && c.ps.vox == vox && !c.ps.counting && !c.ps.have, "on");
  EXPECT(c.ps.n[0] == 4 && c.ps.pixel_type == CUBERILLE_PIX_F32 && std::signbit(c.ps.outside) && c.ps.geo.p2i[0] == 1.0, "the image as described");
  EXPECT(cuberille_set_point_scalars(&c, nullptr, nullptr, 0, 0.0) == CUBERILLE_OK && !c.ps.on && !c.ps.vox, "off");
  // a host image whose copy cannot be had (the allocation drill: no device is touched): from off, the setting stays off and
  // the context holds nothing; as a replacement, the setting stays on with the earlier image, every field of it
  g_fail_alloc_countdown = 0;
  EXPECT(cuberille_set_point_scalars(&c, &d, vox, CUBERILLE_MEM_HOST, 1.0) == CUBERILLE_ERR_HIP && !c.ps.on && !c.ps.vox && !c.ps.copy.p && !c.ps.copy.cap &&
             c.err.find("point scalars") != std::string::npos, "a failed first set: \"%s\"", c.err.c_str());
  EXPECT(device_buffers(&c).size() == 38, "a failed first set leaves a bare context's buffers");
  g_fail_alloc_countdown = -1;
  EXPECT(cuberille_set_point_scalars(&c, &d, vox, CUBERILLE_MEM_DEVICE, -0.0) == CUBERILLE_OK && c.ps.on && c.ps.vox == vox, "on again");
  cuberille_image_desc other = d;
  other.pixel_type = CUBERILLE_PIX_U8;
  other.dims[0] = 9;
  other.spacing[1] = 2.0;
  unsigned char bytes[9 * 4 * 4] = {};
  g_fail_alloc_countdown = 0;
  EXPECT(cuberille_set_point_scalars(&c, &other, bytes, CUBERILLE_MEM_HOST, 5.0) == CUBERILLE_ERR_HIP, "a failed replacement");
  g_fail_alloc_countdown = -1;
  EXPECT(c.ps.on && c.ps.vox == vox && c.ps.n[0] == 4 && c.ps.pixel_type == CUBERILLE_PIX_F32 && std::signbit(c.ps.outside) && c.ps.geo.p2i[4] == 1.0 &&
             !c.ps.copy.p && !c.ps.copy.cap, "a failed replacement leaves the setting as it was: on %d vox %p n %d type %d", (int)c.ps.on, c.ps.vox, c.ps.n[0], c.ps.pixel_type);
  EXPECT(cuberille_set_point_scalars(&c, nullptr, nullptr, 0, 0.0) == CUBERILLE_OK && !c.ps.on && !c.ps.vox, "off once more");
  c.stepMode = 1;
  EXPECT(cuberille_set_point_scalars(&c, &d, vox, CUBERILLE_MEM_DEVICE, 0.0) == CUBERILLE_ERR_STATE && !c.ps.on && c.err == "a step is open on this context", "a step open");
  EXPECT(cuberille_set_point_scalars(nullptr, &d, vox, CUBERILLE_MEM_DEVICE, 0.0) == CUBERILLE_ERR_ARGUMENT, "no context");
}

// rows_home on a bare context: capacities set by hand, no memory behind them
void rows_go_home() {
  for (int on = 0; on < 2; on++) {
    cuberille_ctx c;
    c.ps.on = on != 0;
    c.ps.rows.row.cap = 100;
    c.ps.rows.spare.cap = 1000;
    for (int pass = 0; pass < 2; pass++) {
      rows_home(&c);
      EXPECT(c.ps.rows.row.cap == (on ? 1000u : 100u) && c.ps.rows.spare.cap == (on ? 100u : 1000u), "setting %d pass %d: row %zu spare %zu", on, pass,
             c.ps.rows.row.cap, c.ps.rows.spare.cap);
      EXPECT(!c.ps.rows.row.p && !c.ps.rows.spare.p, "no memory");
    }
    c.ps.rows.row.cap = c.ps.rows.spare.cap = 0;
  }
}

}  // namespace

int main() {
  reservations();
  buffers();
  refusals();
  setter();
  rows_go_home();
  std::printf(failures ? "point_scalars_table: %d check(s) FAILED\n" : "point_scalars_table ok\n", failures);
  return failures ? 1 : 0;
}
